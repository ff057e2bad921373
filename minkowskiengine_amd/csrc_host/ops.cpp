// Operators of the native host layer (see host.hpp): C++ twin of the operator functions of minkowskiengine_amd/backend.py.
// Reference entry points: src/convolution_gpu.cu:45-244, src/convolution_transpose_gpu.cu, src/local_pooling_gpu.cu,
// src/global_pooling_gpu.cu, src/broadcast_gpu.cu, src/pruning_gpu.cu (signatures pybind/extern.hpp:53-392).
#include "host.hpp"

#include <c10/util/intrusive_ptr.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <optional>
#include <stdexcept>

namespace meh {

static void check_feat(const char *name, const Tensor &t) {
  check(t.is_contiguous(), std::string(name) + " must be contiguous");
  check(t.is_cuda(), std::string(name) + " must be CUDA (ROCm) — the MI355X path has no CPU implementation");
  check(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kDouble,
        std::string(name) + " must be float32, bfloat16 or float64");
}

// ---- packed weight images: cached per (weight storage, direction), validated by the tensor's version counter ------------
// (C++ twin of backend._WeightPacker; every stale image of the device is repacked by ONE launch, csrc/pack.hip)
namespace {
struct PackEntry {
  c10::weak_intrusive_ptr<c10::TensorImpl> ref{c10::weak_intrusive_ptr<c10::TensorImpl>(
      c10::intrusive_ptr<c10::TensorImpl>())};
  const void *ptr = nullptr;
  std::vector<int64_t> shape;
  at::ScalarType dtype = at::kFloat;
  int64_t version = -1;
  int64_t epoch = -1;          // g_pack_epoch at pack time (invalidate_packed_weights)
  bool packed_once = false;
  Tensor packed;
  me_pack_job job;
};
typedef std::tuple<const void *, int, bool> PackKey;

struct Packer {
  std::map<PackKey, std::shared_ptr<PackEntry>> entries;
  std::vector<PackEntry *> table_key;
  Tensor table_jobs, table_prefix;
  int64_t table_total = 0;
  std::vector<std::shared_ptr<PackEntry>> table_entries;
};
std::map<int, Packer> g_packers;
// The version counter does not see writes through `.data` (p.data.add_(1) leaves p._version alone): optimizers and
// utilities that update weights that way (Apex / DeepSpeed style, EMA, clipping) call invalidate_packed_weights(), and
// the package does so itself after every torch.optim step (a global step post-hook, __init__.py).  An image is valid
// for (version, epoch); the epoch only grows.  Backward runs on autograd worker threads: one mutex for the packers.
std::atomic<int64_t> g_pack_epoch{0};
std::mutex g_packers_mu;

// version counter and liveness of the tensor an entry was made for (a full view is anchored at its base)
bool entry_alive(const PackEntry &e, int64_t *version) {
  auto strong = e.ref.lock();
  if (!strong) return false;
  if (strong->storage().data() == nullptr) return false;
  const char *p = static_cast<const char *>(strong->storage().data()) + strong->storage_offset() * strong->itemsize();
  if (p != e.ptr) return false;
  *version = (int64_t)strong->version_counter().current_version();
  return true;
}

void pack_one(PackEntry &e, const c10::Device &dev) {
  c10::DeviceGuard guard(dev);
  const me_pack_job &j = e.job;
  if (j.mode == ME_PACK_BF16)
    me_ok(me_conv_pack_weights_bf16(j.w, j.w_is_f32, j.volume, j.c_src, j.c_dst, j.transposed, (uint16_t *)j.wp,
                                    stream_of(dev)));
  else
    me_ok(me_conv_pack_weights_f32x3((const float *)j.w, j.volume, j.c_src, j.c_dst, j.transposed, (uint16_t *)j.wp,
                                     stream_of(dev)));
}
}  // namespace

void invalidate_packed_weights() { g_pack_epoch.fetch_add(1); }

// only the images of the weights at these storage addresses (the optimizer-step hook passes the stepping optimizer's
// own parameters: frozen / teacher networks keep their images)
void invalidate_packed_weights_for(const std::vector<int64_t> &ptrs) {
  std::lock_guard<std::mutex> lk(g_packers_mu);
  for (auto &pk : g_packers)
    for (auto &kv : pk.second.entries)
      if (std::binary_search(ptrs.begin(), ptrs.end(), (int64_t)(intptr_t)kv.second->ptr)) kv.second->epoch = -1;
}

// ... of the weights that live inside one of the byte ranges [begins[i], ends[i]) (sorted, disjoint or nested starts):
// a kernel that is an offset view of a stepping parameter is matched too.  -> (images matched, images cached): a caller
// that matched nothing holds master copies, not the model's tensors, and bumps the global epoch
std::pair<int64_t, int64_t> invalidate_packed_weights_in(const std::vector<int64_t> &begins,
                                                         const std::vector<int64_t> &ends) {
  std::lock_guard<std::mutex> lk(g_packers_mu);
  int64_t matched = 0, total = 0;
  for (auto &pk : g_packers)
    for (auto &kv : pk.second.entries) {
      ++total;
      const int64_t a = (int64_t)(intptr_t)kv.second->ptr;
      auto it = std::upper_bound(begins.begin(), begins.end(), a);
      if (it == begins.begin()) continue;
      const size_t i = (size_t)(it - begins.begin()) - 1;
      if (i < ends.size() && a < ends[i]) {
        kv.second->epoch = -1;
        ++matched;
      }
    }
  return {matched, total};
}

Tensor packed_weights(const Tensor &kernel, int mode, bool transposed, int c_src, int c_dst, int64_t elems) {
  const c10::Device dev = kernel.device();
  std::lock_guard<std::mutex> lk(g_packers_mu);
  const int64_t epoch = g_pack_epoch.load();
  Packer &pk = g_packers[dev.index()];
  const PackKey key(kernel.data_ptr(), mode, transposed);
  const int64_t cur_version = (int64_t)kernel.unsafeGetTensorImpl()->version_counter().current_version();
  std::shared_ptr<PackEntry> ent;
  auto it = pk.entries.find(key);
  int64_t v = 0;
  if (it != pk.entries.end() && entry_alive(*it->second, &v) && it->second->shape == kernel.sizes().vec() &&
      it->second->dtype == kernel.scalar_type()) {
    ent = it->second;
    if (ent->packed_once && ent->version == cur_version && ent->epoch == epoch) return ent->packed;
  } else {
    if (pk.entries.size() > 4096) {
      for (auto i = pk.entries.begin(); i != pk.entries.end();) {
        int64_t vv;
        i = entry_alive(*i->second, &vv) ? std::next(i) : pk.entries.erase(i);
      }
    }
    ent = std::make_shared<PackEntry>();
    // anchor: the base of a full view (a 1x1 convolution passes kernel.unsqueeze(0)), else the tensor itself
    c10::intrusive_ptr<c10::TensorImpl> anchor = kernel.getIntrusivePtr();
    if (kernel.is_view()) {
      const at::TensorBase &base = kernel._base();
      if (base.defined() && base.data_ptr() == kernel.data_ptr() && base.numel() == kernel.numel())
        anchor = base.getIntrusivePtr();
    }
    ent->ref = c10::weak_intrusive_ptr<c10::TensorImpl>(anchor);
    ent->ptr = kernel.data_ptr();
    ent->shape = kernel.sizes().vec();
    ent->dtype = kernel.scalar_type();
    ent->packed = at::empty({elems}, at::TensorOptions().dtype(at::kBFloat16).device(dev));
    std::memset(&ent->job, 0, sizeof(ent->job));
    ent->job.w = kernel.data_ptr();
    ent->job.wp = ent->packed.data_ptr();
    ent->job.volume = kernel.size(0);
    ent->job.c_src = c_src;
    ent->job.c_dst = c_dst;
    ent->job.transposed = transposed ? 1 : 0;
    ent->job.w_is_f32 = kernel.scalar_type() == at::kFloat ? 1 : 0;
    ent->job.mode = mode;
    me_ok(me_conv_pack_job_init(&ent->job));
    pk.entries[key] = ent;
  }
  // a NEW entry is packed on its own, so that the set of established images (and the cached job table) repeats
  if (!ent->packed_once) {
    pack_one(*ent, dev);
    ent->packed_once = true;
    ent->version = cur_version;
    ent->epoch = epoch;
  }
  std::vector<std::pair<std::shared_ptr<PackEntry>, int64_t>> stale;
  for (auto &kv : pk.entries) {
    PackEntry &e = *kv.second;
    if (!e.packed_once) continue;
    int64_t ev = 0;
    if (kv.second == ent) ev = cur_version;
    else if (!entry_alive(e, &ev)) continue;
    if (ev != e.version || e.epoch != epoch) stale.push_back({kv.second, ev});
  }
  if (stale.empty()) return ent->packed;
  if (stale.size() > 1024) {   // (the wanted image is never the one that is dropped)
    const bool wanted_stale = ent->version != cur_version || ent->epoch != epoch;
    stale.erase(stale.begin(), stale.end() - 1024);
    if (wanted_stale && std::none_of(stale.begin(), stale.end(), [&](auto &s) { return s.first == ent; }))
      stale.front() = {ent, cur_version};
  }
  if (stale.size() == 1) {
    pack_one(*stale[0].first, dev);
    stale[0].first->version = stale[0].second;
    stale[0].first->epoch = epoch;
    return ent->packed;
  }
  std::vector<PackEntry *> tk;
  for (auto &s : stale) tk.push_back(s.first.get());
  if (tk != pk.table_key) {
    std::vector<me_pack_job> jobs;
    std::vector<int64_t> prefix{0};
    for (auto &s : stale) {
      jobs.push_back(s.first->job);
      prefix.push_back(prefix.back() + s.first->job.threads);
    }
    Tensor jb = at::empty({(int64_t)(jobs.size() * sizeof(me_pack_job))}, at::TensorOptions().dtype(at::kByte));
    std::memcpy(jb.data_ptr(), jobs.data(), jobs.size() * sizeof(me_pack_job));
    pk.table_jobs = jb.to(dev);
    pk.table_prefix = at::tensor(prefix, at::TensorOptions().dtype(at::kLong)).to(dev);
    pk.table_total = prefix.back();
    pk.table_key = tk;
    pk.table_entries.clear();
    for (auto &s : stale) pk.table_entries.push_back(s.first);
  }
  {
    c10::DeviceGuard guard(dev);
    me_ok(me_conv_pack_weights_multi((const me_pack_job *)pk.table_jobs.data_ptr(), (int)stale.size(),
                                     ptr<int64_t>(pk.table_prefix), pk.table_total, stream_of(dev)));
  }
  for (auto &s : stale) {
    s.first->version = s.second;
    s.first->epoch = epoch;
  }
  return ent->packed;
}

// ---- per-launch timing (bench.py) ---------------------------------------------------------------------------------------------
namespace {
struct TimedLaunch {
  std::string name;
  hipEvent_t a, b;
  double flops;
};
bool g_timing = false;
std::vector<TimedLaunch> g_timed;

struct ScopedTimer {   // records an event pair around the launches of its scope when timing is on; a roctx range always
  bool on;                // (when ME_AMD_ROCTX=1: "me:conv_forward" / "me:conv_dgrad" / "me:conv_wgrad")
                          // In the two-launch backward order (conv_backward_km) "conv_wgrad" is the first pass of the weight
                          // gradient only; its reduce is the tail of the input-gradient launch and counts under "conv_dgrad".
  TimedLaunch t;
  hipStream_t st;
  std::string rx_name;
  RoctxRange rx;
  ScopedTimer(const char *name, double flops, void *stream)
      : on(g_timing), st((hipStream_t)stream), rx_name(std::string("me:") + name), rx(rx_name.c_str()) {
    if (!on) return;
    t.name = name;
    t.flops = flops;
    (void)hipEventCreate(&t.a);
    (void)hipEventCreate(&t.b);
    (void)hipEventRecord(t.a, st);
  }
  ~ScopedTimer() {
    if (!on) return;
    (void)hipEventRecord(t.b, st);
    g_timed.push_back(t);
  }
};
}  // namespace

void timing_enable(bool on) { g_timing = on; }

std::vector<std::tuple<std::string, double, double>> timing_records(bool clear) {
  std::vector<std::tuple<std::string, double, double>> out;
  for (auto &t : g_timed) {
    (void)hipEventSynchronize(t.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t.a, t.b);
    out.emplace_back(t.name, (double)ms, t.flops);
  }
  if (clear) {
    for (auto &t : g_timed) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    g_timed.clear();
  }
  return out;
}

// ---- statistics a convolution leaves behind for the batch norm that follows (me_conv_target_bf16_stats) ----------------
// Keyed by the output's storage address; valid for THAT TensorImpl at THAT version only (a recycled address, a view, an
// in-place update or a channel slice misses and bn_stats reads the matrix).  Consumed by the first bn_stats on it.
namespace {
struct BnPartials {
  c10::weak_intrusive_ptr<c10::TensorImpl> owner;
  uint32_t version;
  Tensor part;   // [2][tiles][c] float
  int tile_rows;
};
std::unordered_map<const void *, BnPartials> g_bn_partials;
std::mutex g_bn_partials_mu;
thread_local bool g_conv_bn_stats_hint = false;   // per thread: a loader thread (ScenePrefetcher) never sees the training thread's flag
int g_conv_bn_stats_enabled = -1;   // -1: Policy (ME_AMD_CONV_BN_STATS), 0 / 1: set_conv_bn_stats (tests)

void bn_partials_put(const Tensor &out, const Tensor &part, int tile_rows) {
  std::lock_guard<std::mutex> lk(g_bn_partials_mu);
  if (g_bn_partials.size() > 32) {    // outputs that were never normalised (their tensors are long gone)
    for (auto it = g_bn_partials.begin(); it != g_bn_partials.end();)
      it = it->second.owner.expired() ? g_bn_partials.erase(it) : std::next(it);
  }
  g_bn_partials.erase(out.data_ptr());
  g_bn_partials.emplace(out.data_ptr(), BnPartials{c10::weak_intrusive_ptr<c10::TensorImpl>(out.getIntrusivePtr()),
                                                   out._version(), part, tile_rows});
}

bool bn_partials_take(const Tensor &x, Tensor &part, int &tile_rows) {
  std::lock_guard<std::mutex> lk(g_bn_partials_mu);
  auto it = g_bn_partials.find(x.data_ptr());
  if (it == g_bn_partials.end()) return false;
  BnPartials e = std::move(it->second);
  g_bn_partials.erase(it);
  auto owner = e.owner.lock();
  if (!owner || owner.get() != x.unsafeGetTensorImpl() || x._version() != e.version) return false;
  if (e.part.size(2) != x.size(1)) return false;
  part = e.part;
  tile_rows = e.tile_rows;
  return true;
}
}  // namespace

void conv_bn_stats_hint(bool flag) { g_conv_bn_stats_hint = flag; }
void set_conv_bn_stats(int enabled) { g_conv_bn_stats_enabled = enabled; }
static bool conv_bn_stats_enabled() {
  return g_conv_bn_stats_enabled >= 0 ? g_conv_bn_stats_enabled != 0 : Policy::get().conv_bn_stats;
}

// ---- gradient destinations (distributed.GradientArena) ---------------------------------------------------------------------
// A parameter's gradient can be BORN in a caller-provided buffer — a slice of one flat all-reduce buffer per dtype — instead
// of a fresh allocation: the weight-gradient / batch-norm backward kernels write there, autograd's AccumulateGrad takes the
// returned alias as p.grad without a copy, and the data-parallel exchange is one RCCL all-reduce over the flat buffer (no
// per-parameter hooks, no bucket copies: torch DDP costs this host-bound step 1.7 ms on ONE rank).  Keyed by the
// parameter's storage address; fp32 only (the dtype the kernels accumulate in).
// An entry is used ONCE per arming (GradientArena.zero_grad arms all of them): a second backward pass before the next
// zero_grad — a gradient-accumulation window — gets fresh tensors, which autograd then ADDS to p.grad (the slice); writing
// into the slice again would destroy what it has accumulated.
namespace {
struct GradDest {
  Tensor dest;
  bool armed;
};
std::unordered_map<const void *, GradDest> g_grad_dest;
std::mutex g_grad_dest_mu;
}  // namespace

void set_grad_destination(const Tensor &param, const Tensor &dest) {
  std::lock_guard<std::mutex> lk(g_grad_dest_mu);
  if (dest.defined()) g_grad_dest[param.data_ptr()] = GradDest{dest, false};
  else g_grad_dest.erase(param.data_ptr());
}
void arm_grad_destinations() {
  std::lock_guard<std::mutex> lk(g_grad_dest_mu);
  for (auto &kv : g_grad_dest) kv.second.armed = true;
}
void arm_grad_destinations_for(const std::vector<int64_t> &ptrs) {   // one arena's own parameters
  std::lock_guard<std::mutex> lk(g_grad_dest_mu);
  for (int64_t a : ptrs) {
    auto it = g_grad_dest.find(reinterpret_cast<const void *>((uintptr_t)a));
    if (it != g_grad_dest.end()) it->second.armed = true;
  }
}
void drop_grad_destinations(const std::vector<int64_t> &ptrs) {
  std::lock_guard<std::mutex> lk(g_grad_dest_mu);
  for (int64_t a : ptrs) g_grad_dest.erase(reinterpret_cast<const void *>((uintptr_t)a));
}
void clear_grad_destinations() {
  std::lock_guard<std::mutex> lk(g_grad_dest_mu);
  g_grad_dest.clear();
}
// a FRESH alias (its own TensorImpl: AccumulateGrad steals a gradient only when nobody else holds it) of the registered
// buffer in `shape`, or an undefined tensor
Tensor grad_destination(const Tensor &param, at::IntArrayRef shape) {
  if (!param.defined()) return Tensor();
  std::lock_guard<std::mutex> lk(g_grad_dest_mu);
  auto it = g_grad_dest.find(param.data_ptr());
  if (it == g_grad_dest.end() || !it->second.armed) return Tensor();
  const Tensor &d = it->second.dest;
  int64_t n = 1;
  for (auto v : shape) n *= v;
  if (d.scalar_type() != at::kFloat || d.numel() != n || d.device() != param.device()) return Tensor();
  it->second.armed = false;
  return d.view(shape);
}

// ---- convolution ----------------------------------------------------------------------------------------------------------
// dst[t] = sum over plan entries of src[s] @ W[k]; transposed (dgrad): W[k] = kernel[k]^T
// tail (conv_backward_km's two-launch order): the launch is the input gradient of a split-fp32 layer and carries the
// reduce of that layer's weight gradient behind its tiles (me_conv_dgrad_reduce_tail_f32x3)
struct ReduceTail {
  const int64_t *koffs;   // host pair offsets
  Tensor ws;              // the partial images me_conv_wgrad_partials_f32 wrote
  Tensor grad_w;
};

static Tensor conv_target(const Tensor &src, const Tensor &kernel, KernelMap &km, const std::string &target, int64_t n_tgt,
                          bool transposed, const ReduceTail *tail = nullptr) {
  const c10::Device dev = src.device();
  const int64_t volume = kernel.size(0);
  const int c_src = (int)(transposed ? kernel.size(2) : kernel.size(1));
  const int c_dst = (int)(transposed ? kernel.size(1) : kernel.size(2));
  const bool bf16 = src.scalar_type() == at::kBFloat16;
  Tensor out = at::empty({n_tgt, c_dst}, src.options());
  if (n_tgt == 0) return out;
  if (src.scalar_type() == at::kDouble) {
    // float64 features (the reference's double instantiation, src/convolution_gpu.cu:137-155 — its gradcheck dtype):
    // csrc/f64.hip, plain double FMAs on the neighbour table; no plan, no packed weights
    check(kernel.scalar_type() == at::kDouble, "float64 features need a float64 kernel");
    Tensor tbl = km.table(target);
    Tensor w = kernel.contiguous();
    c10::DeviceGuard guard(dev);
    void *st = stream_of(dev);
    ScopedTimer tm(transposed ? "conv_dgrad" : "conv_forward", g_timing ? 2.0 * (double)km.n_pairs() * c_src * c_dst : 0.0, st);
    me_ok(me_conv_target_f64(ptr<double>(src), src.size(0), c_src, ptr<double>(w), transposed ? 1 : 0, volume, c_dst,
                             ptr<int32_t>(tbl), ptr<double>(out), n_tgt, st));
    return out;
  }
  if (bf16 && c_src == 8 && src.size(0) < (1ll << 28) && me_conv_stem_use_bf16(n_tgt, volume, c_src, c_dst)) {
    // at most 8 source channels (a stem): four offsets per MFMA step straight off the neighbour table and the layer's own
    // kernel tensor — no tile plan, no packed image (csrc/conv_stem.hip)
    check(kernel.scalar_type() == at::kFloat || kernel.scalar_type() == at::kBFloat16, "kernel must be float32 or bfloat16");
    auto tp = km.table_pos(target);
    Tensor w = kernel.contiguous();
    c10::DeviceGuard guard(dev);
    void *st = stream_of(dev);
    const int tile_rows = me_conv_stem_tile_rows();
    const bool want_stats = !transposed && target == "out" && g_conv_bn_stats_hint && conv_bn_stats_enabled();
    Tensor part;
    int64_t tiles = 0;
    if (want_stats) {
      tiles = (n_tgt + tile_rows - 1) / tile_rows;
      part = at::empty({2, tiles, (int64_t)c_dst}, at::TensorOptions().dtype(at::kFloat).device(dev));
    }
    {
      ScopedTimer tm(transposed ? "conv_dgrad" : "conv_forward", g_timing ? 2.0 * (double)km.n_pairs() * c_src * c_dst : 0.0, st);
      me_ok(me_conv_stem_bf16(ptr<uint16_t>(src), src.size(0), c_src, w.data_ptr(), w.scalar_type() == at::kFloat ? 1 : 0,
                              transposed ? 1 : 0, volume, c_dst, ptr<int32_t>(tp.first), nullptr, ptr<int32_t>(tp.second),
                              ptr<uint16_t>(out), n_tgt, want_stats ? ptr<float>(part) : nullptr,
                              want_stats ? ptr<float>(part) + tiles * c_dst : nullptr, st));
    }
    if (want_stats) bn_partials_put(out, part, tile_rows);
    return out;
  }
  // (a forward launch whose batch-norm statistics are wanted keeps the tile-plan kernel — which leaves them behind — on
  // small maps: ConvCfg::rowwise_min_rows_with_stats)
  const bool stats_wanted = bf16 && !transposed && target == "out" && g_conv_bn_stats_hint && conv_bn_stats_enabled();
  const ConvCfg &cfg0 = km.conv_cfg(target, n_tgt, c_src, c_dst, bf16);
  const ConvCfg &cfg = (cfg0.rowwise && stats_wanted && n_tgt < Policy::get().rowwise_min_rows_with_stats)
                           ? km.conv_cfg(target, n_tgt, c_src, c_dst, bf16, /*no_rowwise=*/true)
                           : cfg0;
  c10::DeviceGuard guard(dev);
  void *st = stream_of(dev);
  auto timed_name = transposed ? "conv_dgrad" : "conv_forward";
  const double flops = g_timing ? 2.0 * (double)km.n_pairs() * c_src * c_dst : 0.0;
  if (cfg.rowwise) {
    // exactly one pair per target row (K = 1 layers — the reference's input.F.mm(kernel) —, the fine side of a
    // kernel_size == stride map): rows stream through the MFMA registers, no plan (csrc/conv_rowwise.hip)
    check(kernel.scalar_type() == at::kFloat || kernel.scalar_type() == at::kBFloat16, "kernel must be float32 or bfloat16");
    Tensor packed;
    if (Policy::get().pack_cache) {
      packed = packed_weights(kernel, ME_PACK_BF16, transposed, c_src, c_dst, cfg.elems);
    } else {
      packed = at::empty({cfg.elems}, at::TensorOptions().dtype(at::kBFloat16).device(dev));
      me_ok(me_conv_pack_weights_bf16(kernel.data_ptr(), kernel.scalar_type() == at::kFloat ? 1 : 0, volume, c_src, c_dst,
                                      transposed ? 1 : 0, ptr<uint16_t>(packed), st));
    }
    const Tensor &src_rows = target == "out" ? km.in_pairs_buf : km.out_pairs_buf;
    const Tensor &tgt_rows = target == "out" ? km.out_pairs_buf : km.in_pairs_buf;
    ScopedTimer tm(timed_name, flops, st);
    me_ok(me_conv_rowwise_bf16(ptr<uint16_t>(src), src.size(0), c_src, ptr<uint16_t>(packed), km.volume, c_dst,
                               ptr<int32_t>(src_rows), ptr<int32_t>(tgt_rows), ptr<int64_t>(km.k_offsets_dev), n_tgt,
                               ptr<uint16_t>(out), n_tgt, st));
    return out;
  }
  if (cfg.halo) {
    // output-stationary launch on the LDS-staged source halo (csrc/conv_halo.hip): the same packed weights; the
    // batch-norm partials per halo tile
    check(kernel.scalar_type() == at::kFloat || kernel.scalar_type() == at::kBFloat16, "kernel must be float32 or bfloat16");
    const HaloPlan &h = *cfg.halo;
    Tensor packed;
    if (Policy::get().pack_cache) {
      packed = packed_weights(kernel, ME_PACK_BF16, transposed, c_src, c_dst, cfg.elems);
    } else {
      packed = at::empty({cfg.elems}, at::TensorOptions().dtype(at::kBFloat16).device(dev));
      me_ok(me_conv_pack_weights_bf16(kernel.data_ptr(), kernel.scalar_type() == at::kFloat ? 1 : 0, volume, c_src, c_dst,
                                      transposed ? 1 : 0, ptr<uint16_t>(packed), st));
    }
    const bool want_stats = !transposed && target == "out" && g_conv_bn_stats_hint && conv_bn_stats_enabled();
    Tensor part;
    int64_t tiles = 0;
    if (want_stats) {
      tiles = (n_tgt + h.tile_rows - 1) / h.tile_rows;
      part = at::empty({2, tiles, (int64_t)c_dst}, at::TensorOptions().dtype(at::kFloat).device(dev));
    }
    {
      ScopedTimer tm(timed_name, flops, st);
      me_ok(me_conv_halo_bf16(ptr<uint16_t>(src), src.size(0), c_src, ptr<uint16_t>(packed), km.volume, c_dst,
                              ptr<int32_t>(h.halo_cnt), ptr<int32_t>(h.halo_rows), ptr<uint16_t>(h.lidx),
                              ptr<uint32_t>(h.kmask), ptr<int32_t>(h.tbl), ptr<int32_t>(h.col_order),
                              ptr<int32_t>(h.out_order), ptr<uint16_t>(out), n_tgt, h.tile_rows, h.s_cap,
                              want_stats ? ptr<float>(part) : nullptr, want_stats ? ptr<float>(part) + tiles * c_dst : nullptr,
                              st));
    }
    if (want_stats) bn_partials_put(out, part, h.tile_rows);
    return out;
  }
  const Plan &p = *cfg.plan;
  if (bf16) {
    check(kernel.scalar_type() == at::kFloat || kernel.scalar_type() == at::kBFloat16, "kernel must be float32 or bfloat16");
    Tensor packed;
    if (Policy::get().pack_cache) {
      packed = packed_weights(kernel, ME_PACK_BF16, transposed, c_src, c_dst, cfg.elems);
    } else {
      packed = at::empty({cfg.elems}, at::TensorOptions().dtype(at::kBFloat16).device(dev));
      me_ok(me_conv_pack_weights_bf16(kernel.data_ptr(), kernel.scalar_type() == at::kFloat ? 1 : 0, volume, c_src, c_dst,
                                      transposed ? 1 : 0, ptr<uint16_t>(packed), st));
    }
    // One entry point for the bf16 forward / dgrad launch (me_conv_target_bf16_ex): batch fusion, the batch-norm
    // statistics of the output (forward launches only: target "out", weights not transposed — the input gradient feeds
    // no batch norm) and split-K (small maps: offset groups through an fp32 workspace) by argument.
    const bool want_stats = !transposed && target == "out" && g_conv_bn_stats_hint && conv_bn_stats_enabled() &&
                            me_conv_stats_supported_bf16(c_src, c_dst);
    Tensor part, ws;
    int64_t tiles = 0;
    if (want_stats) {
      // the tiles' (mean, M2) partials ride along with the output (bn_stats consumes them: bn_partials_take)
      tiles = (n_tgt + cfg.tile_rows - 1) / cfg.tile_rows;
      part = at::empty({2, tiles, (int64_t)c_dst}, at::TensorOptions().dtype(at::kFloat).device(dev));
    }
    if (cfg.split_k > 1)
      ws = at::empty({me_conv_splitk_workspace_bytes(n_tgt, cfg.tile_rows, c_dst, cfg.split_k) / 4},
                     at::TensorOptions().dtype(at::kFloat).device(dev));
    {
      ScopedTimer tm(timed_name, flops, st);
      me_ok(me_conv_target_bf16_ex(
          ptr<uint16_t>(src), src.size(0), c_src, ptr<uint16_t>(packed), km.volume, c_dst, ptr<int32_t>(p.plan_src),
          ptr<int32_t>(p.plan_dst), ptr<int32_t>(p.batch_desc), ptr<int32_t>(p.tile_bptr), ptr<int32_t>(cfg.order),
          ptr<uint16_t>(out), n_tgt, cfg.tile_rows, cfg.batch_groups, cfg.fuse ? 1 : 0, cfg.split_k, vptr(ws),
          want_stats ? ptr<float>(part) : nullptr, want_stats ? ptr<float>(part) + tiles * c_dst : nullptr, st));
    }
    if (want_stats) bn_partials_put(out, part, cfg.tile_rows);
    return out;
  }
  check(kernel.scalar_type() == at::kFloat, "float32 features need a float32 kernel");
  if (cfg.split) {
    Tensor packed;
    if (Policy::get().pack_cache) {
      packed = packed_weights(kernel, ME_PACK_F32X3, transposed, c_src, c_dst, cfg.elems);
    } else {
      packed = at::empty({cfg.elems}, at::TensorOptions().dtype(at::kBFloat16).device(dev));
      me_ok(me_conv_pack_weights_f32x3(ptr<float>(kernel), volume, c_src, c_dst, transposed ? 1 : 0, ptr<uint16_t>(packed),
                                       st));
    }
    ScopedTimer tm(timed_name, flops, st);   // (with a tail, "conv_dgrad" includes the weight gradient's reduce)
    if (tail != nullptr)
      me_ok(me_conv_dgrad_reduce_tail_f32x3(ptr<float>(src), src.size(0), c_src, ptr<uint16_t>(packed), km.volume, c_dst,
                                            ptr<int32_t>(p.plan_src), ptr<int32_t>(p.plan_dst), ptr<int32_t>(p.batch_desc),
                                            ptr<int32_t>(p.tile_bptr), ptr<int32_t>(cfg.order), ptr<float>(out), n_tgt,
                                            cfg.tile_rows, cfg.batch_groups, tail->koffs, ptr<int64_t>(km.k_offsets_dev),
                                            vptr(tail->ws), tail->ws.numel(), ptr<float>(tail->grad_w), st));
    else
      me_ok(me_conv_target_f32x3(ptr<float>(src), src.size(0), c_src, ptr<uint16_t>(packed), km.volume, c_dst,
                                 ptr<int32_t>(p.plan_src), ptr<int32_t>(p.plan_dst), ptr<int32_t>(p.batch_desc),
                                 ptr<int32_t>(p.tile_bptr), ptr<int32_t>(cfg.order), ptr<float>(out), n_tgt, cfg.tile_rows,
                                 cfg.batch_groups, st));
    return out;
  }
  check(tail == nullptr, "reduce tail on a launch that is not the split fp32 kernel");
  Tensor packed = at::empty({cfg.elems}, at::TensorOptions().dtype(at::kFloat).device(dev));
  me_ok(me_conv_pack_weights_f32(ptr<float>(kernel), volume, c_src, c_dst, transposed ? 1 : 0, ptr<float>(packed), st));
  ScopedTimer tm(timed_name, flops, st);
  me_ok((cfg.fuse && Policy::get().f32_fuse ? me_conv_target_f32_fused : me_conv_target_f32)(ptr<float>(src), src.size(0), c_src, ptr<float>(packed), km.volume, c_dst,
                           ptr<int32_t>(p.plan_src), ptr<int32_t>(p.plan_dst), ptr<int32_t>(p.batch_desc),
                           ptr<int32_t>(p.tile_bptr), ptr<int32_t>(cfg.order), ptr<float>(out), n_tgt, cfg.tile_rows,
                           cfg.batch_groups, st));
  return out;
}

Tensor conv_forward_km(const Tensor &in_feat, const Tensor &kernel, KernelMap &km) {
  return conv_target(in_feat, kernel, km, "out", km.n_out, false);
}

std::pair<Tensor, Tensor> conv_backward_km(const Tensor &in_feat, Tensor grad_out, const Tensor &kernel, KernelMap &km,
                                           bool need_grad_in) {
  const c10::Device dev = in_feat.device();
  const int64_t volume = kernel.size(0);
  const int c_in = (int)kernel.size(1), c_out = (int)kernel.size(2);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  const bool bf16 = in_feat.scalar_type() == at::kBFloat16;
  // Two-launch order (split fp32 layers whose input gradient is the wave-specialised split kernel, both gradients
  // wanted): the weight gradient's partial images FIRST, then the input gradient, whose trailing workgroups reduce
  // the images into grad_w on CUs that have run out of tiles — no reduce launch.  Everything else: input gradient,
  // weight gradient, reduce, as ever.
  bool two_launch = false;
  if (need_grad_in && in_feat.scalar_type() == at::kFloat && kernel.scalar_type() == at::kFloat && km.n_in > 0 &&
      me_conv_dgrad_reduce_tail_supported(c_in, c_out, volume, km.n_pairs())) {
    const ConvCfg &dc = km.conv_cfg("in", km.n_in, c_out, c_in, false);
    two_launch = dc.split && !dc.rowwise && !dc.halo && dc.plan != nullptr;
  }
  // dgrad: the same target-stationary kernel; the weights are packed transposed per offset
  Tensor grad_in;
  if (need_grad_in && !two_launch) grad_in = conv_target(grad_out, kernel, km, "in", km.n_in, true);
  if (in_feat.scalar_type() == at::kDouble) {   // csrc/f64.hip: sequential double sums over the pairs of each offset
    check(kernel.scalar_type() == at::kDouble, "float64 features need a float64 kernel");
    Tensor gw = at::empty(kernel.sizes(), kernel.options());
    Tensor x = in_feat.contiguous(), dy = grad_out.contiguous();
    c10::DeviceGuard guard(dev);
    me_ok(me_conv_wgrad_f64(ptr<double>(x), c_in, ptr<double>(dy), c_out, ptr<int32_t>(km.in_pairs_buf),
                            ptr<int32_t>(km.out_pairs_buf), ptr<int64_t>(km.k_offsets_dev), volume, ptr<double>(gw),
                            stream_of(dev)));
    return {grad_in, gw};
  }
  // wgrad: always accumulated and reduced in fp32; handed back in the kernel's dtype
  Tensor grad_w = kernel.scalar_type() == at::kFloat ? grad_destination(kernel, kernel.sizes()) : Tensor();
  if (!grad_w.defined()) grad_w = at::empty(kernel.sizes(), at::TensorOptions().dtype(at::kFloat).device(dev));
  const WgradCfg &w = km.wgrad_cfg(c_in, c_out, bf16);
  Tensor ws = workspace(w.ws_bytes, dev);
  if (two_launch) {
    {
      c10::DeviceGuard guard(dev);
      void *st = stream_of(dev);
      ScopedTimer tm("conv_wgrad", g_timing ? 2.0 * (double)km.n_pairs() * c_in * c_out : 0.0, st);
      me_ok(me_conv_wgrad_partials_f32(ptr<float>(in_feat), in_feat.size(0), c_in, ptr<float>(grad_out), grad_out.size(0),
                                       c_out, ptr<int32_t>(km.in_pairs_buf), ptr<int32_t>(km.out_pairs_buf), w.koffs.data(),
                                       ptr<int64_t>(km.k_offsets_dev), volume, vptr(ws), ws.numel(), st));
    }
    const ReduceTail tail{w.koffs.data(), ws, grad_w};
    grad_in = conv_target(grad_out, kernel, km, "in", km.n_in, true, &tail);
    return {grad_in, grad_w};
  }
  {
    c10::DeviceGuard guard(dev);
    void *st = stream_of(dev);
    ScopedTimer tm("conv_wgrad", g_timing ? 2.0 * (double)km.n_pairs() * c_in * c_out : 0.0, st);
    if (bf16)
      me_ok(me_conv_wgrad_bf16(ptr<uint16_t>(in_feat), in_feat.size(0), c_in, ptr<uint16_t>(grad_out), grad_out.size(0),
                               c_out, ptr<int32_t>(km.in_pairs_buf), ptr<int32_t>(km.out_pairs_buf), w.koffs.data(),
                               ptr<int64_t>(km.k_offsets_dev), volume, ptr<float>(grad_w), vptr(ws), ws.numel(), st));
    else
      me_ok(me_conv_wgrad_f32(ptr<float>(in_feat), in_feat.size(0), c_in, ptr<float>(grad_out), grad_out.size(0), c_out,
                              ptr<int32_t>(km.in_pairs_buf), ptr<int32_t>(km.out_pairs_buf), w.koffs.data(),
                              ptr<int64_t>(km.k_offsets_dev), volume, ptr<float>(grad_w), vptr(ws), ws.numel(), st));
  }
  if (kernel.scalar_type() != at::kFloat) grad_w = grad_w.to(kernel.scalar_type());
  return {grad_in, grad_w};
}

std::shared_ptr<KernelMap> prepare_conv(const Tensor &in_feat, const Tensor &kernel, const ivec &kernel_size,
                                        const ivec &kernel_stride, const ivec &kernel_dilation, int region_type,
                                        bool expand_coordinates, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
                                        CoordinateMapManager *manager, bool transpose, const ivec &offsets) {
  check_feat("in_feat", in_feat);
  check_feat("kernel", kernel);
  check(in_feat.dim() == 2, "in_feat.dim() must be 2");
  check(kernel.dim() == 3, "kernel.dim() must be 3");
  check(in_feat.size(1) == kernel.size(1), "Input feature size and kernel size mismatch");
  const KeyT &ik = in_key->get();
  check(manager->exists(ik), "coordinate map not found");
  check(in_feat.size(0) == manager->get(ik)->n, "Invalid in_feat size");
  if (!out_key->key_set) {
    const ivec &ts = ik.first;
    if (!transpose) {
      if (expand_coordinates) {
        // src/convolution_cpu.cpp:79-103: every kernel offset around every input voxel that falls on the output grid
        ivec out_ts(ts.size());
        for (size_t i = 0; i < ts.size(); ++i) out_ts[i] = ts[i] * kernel_stride[i];
        auto r = manager->stride_region(ik, kernel_size, kernel_dilation, region_type, out_ts, true, false, &ts, offsets);
        out_key->set_key(r.first.first, r.first.second);
      } else {
        KeyT ok = manager->stride(ik, kernel_stride, "");
        out_key->set_key(ok.first, ok.second);
      }
    } else {
      // src/convolution_transpose_cpu.cpp:76-97: out tensor stride = in / stride
      ivec out_ts(ts.size());
      for (size_t i = 0; i < ts.size(); ++i) {
        check(kernel_stride[i] > 0 && ts[i] % kernel_stride[i] == 0, "Invalid up stride on tensor stride");
        out_ts[i] = ts[i] / kernel_stride[i];
      }
      auto r = manager->stride_region(ik, kernel_size, kernel_dilation, region_type, out_ts, expand_coordinates, true,
                                      nullptr, offsets);
      out_key->set_key(r.first.first, r.first.second);
    }
  }
  return manager->kernel_map(ik, out_key->get(), kernel_size, kernel_stride, kernel_dilation, region_type, transpose, false,
                             offsets);
}

// ---- pooling / broadcast ----------------------------------------------------------------------------------------------------
enum { LOCAL_SUM = 0, LOCAL_AVG = 1, LOCAL_MAX = 2 };
static int global_mode(int pooling_mode) {   // -> 0 sum / 1 avg / 2 max (PoolingMode values 3..11)
  check(pooling_mode >= 3 && pooling_mode <= 11, "Invalid pooling mode");
  return (pooling_mode - 3) % 3;
}

static std::pair<Tensor, Tensor> pool_sum(const Tensor &src, const Tensor &tbl, int64_t n_tgt, int64_t volume,
                                          const Tensor &src_count, bool average, bool want_count) {
  const c10::Device dev = src.device();
  const int c = (int)src.size(1);
  Tensor out = at::empty({n_tgt, c}, src.options());
  Tensor cnt;
  if (want_count) cnt = at::empty({n_tgt > 0 ? n_tgt : 1}, at::TensorOptions().dtype(at::kFloat).device(dev)).narrow(0, 0, n_tgt);
  if (src_count.defined()) check(src_count.scalar_type() == at::kFloat, "num_nonzero must be float32");
  c10::DeviceGuard guard(dev);
  if (src.scalar_type() == at::kDouble)
    me_ok(me_pool_sum_f64(ptr<double>(src), c, ptr<int32_t>(tbl), n_tgt, volume, ptr<float>(src_count), average ? 1 : 0,
                          ptr<double>(out), ptr<float>(cnt), stream_of(dev)));
  else if (src.scalar_type() == at::kBFloat16)
    me_ok(me_pool_sum_bf16(ptr<uint16_t>(src), c, ptr<int32_t>(tbl), n_tgt, volume, ptr<float>(src_count), average ? 1 : 0,
                           ptr<uint16_t>(out), ptr<float>(cnt), stream_of(dev)));
  else
    me_ok(me_pool_sum_f32(ptr<float>(src), c, ptr<int32_t>(tbl), n_tgt, volume, ptr<float>(src_count), average ? 1 : 0,
                          ptr<float>(out), ptr<float>(cnt), stream_of(dev)));
  return {out, cnt};
}

static void prepare_pool(const Tensor &in_feat, const ivec &kernel_stride, CoordinateMapKey *in_key,
                         CoordinateMapKey *out_key, CoordinateMapManager *mgr, bool transpose) {
  check_feat("in_feat", in_feat);
  check(in_feat.dim() == 2, "in_feat.dim() must be 2");
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik), "coordinate map not found");
  check(in_feat.size(0) == mgr->get(ik)->n, "Invalid in_feat size");
  if (out_key->key_set) return;
  if (!transpose) {
    KeyT ok = mgr->stride(ik, kernel_stride, "");
    out_key->set_key(ok.first, ok.second);
  } else {
    ivec out_ts(ik.first.size());
    for (size_t i = 0; i < out_ts.size(); ++i) {
      check(kernel_stride[i] > 0 && ik.first[i] % kernel_stride[i] == 0, "Invalid up stride on tensor stride");
      out_ts[i] = ik.first[i] / kernel_stride[i];
    }
    check(mgr->exists(KeyT(out_ts, "")), "pooling transpose needs an existing output map");
    out_key->set_key(out_ts, "");
  }
}

std::pair<Tensor, Tensor> local_pooling_forward(const Tensor &in_feat, const ivec &ks, const ivec &st, const ivec &dl,
                                                int region_type, int pooling_mode, CoordinateMapKey *in_key,
                                                CoordinateMapKey *out_key, CoordinateMapManager *mgr,
                                                const ivec &offsets) {
  prepare_pool(in_feat, st, in_key, out_key, mgr, false);
  auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, region_type, false, true, offsets);
  if (pooling_mode == LOCAL_MAX) {
    const c10::Device dev = in_feat.device();
    const int c = (int)in_feat.size(1);
    Tensor out = at::empty({km->n_out, c}, in_feat.options());
    Tensor mask = empty_i32({km->n_out, c}, dev);
    Tensor tbl = km->table("out");
    c10::DeviceGuard guard(dev);
    if (in_feat.scalar_type() == at::kDouble)
      me_ok(me_pool_max_f64(ptr<double>(in_feat), c, ptr<int32_t>(tbl), km->n_out, km->volume, ptr<double>(out),
                            ptr<int32_t>(mask), stream_of(dev)));
    else if (in_feat.scalar_type() == at::kBFloat16)
      me_ok(me_pool_max_bf16(ptr<uint16_t>(in_feat), c, ptr<int32_t>(tbl), km->n_out, km->volume, ptr<uint16_t>(out),
                             ptr<int32_t>(mask), stream_of(dev)));
    else
      me_ok(me_pool_max_f32(ptr<float>(in_feat), c, ptr<int32_t>(tbl), km->n_out, km->volume, ptr<float>(out),
                            ptr<int32_t>(mask), stream_of(dev)));
    return {out, mask};
  }
  check(pooling_mode == LOCAL_SUM || pooling_mode == LOCAL_AVG, "Invalid pooling mode");
  const bool avg = pooling_mode == LOCAL_AVG;
  auto r = pool_sum(in_feat, km->table("out"), km->n_out, km->volume, Tensor(), avg, avg);
  if (!r.second.defined()) r.second = at::empty({0}, at::TensorOptions().dtype(at::kFloat).device(in_feat.device()));
  return r;
}

Tensor local_pooling_backward(const Tensor &in_feat, Tensor grad_out, const Tensor &num_nonzero, const ivec &ks,
                              const ivec &st, const ivec &dl, int region_type, int pooling_mode,
                              CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr,
                              const ivec &offsets) {
  check_feat("in_feat", in_feat);
  grad_out = grad_out.contiguous();
  check_feat("grad_out_feat", grad_out);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, region_type, false, true, offsets);
  check(grad_out.size(0) == km->n_out, "Invalid grad_out size");
  if (pooling_mode == LOCAL_MAX) {
    const c10::Device dev = in_feat.device();
    const int c = (int)in_feat.size(1);
    check(num_nonzero.scalar_type() == at::kInt, "the max-pooling mask must be int32");
    Tensor grad_in = at::empty({km->n_in, c}, in_feat.options());
    Tensor tbl = km->table("in");
    c10::DeviceGuard guard(dev);
    if (in_feat.scalar_type() == at::kDouble)
      me_ok(me_pool_max_backward_f64(ptr<double>(grad_out), c, ptr<int32_t>(tbl), km->n_in, km->volume,
                                     ptr<int32_t>(num_nonzero), ptr<double>(grad_in), stream_of(dev)));
    else if (in_feat.scalar_type() == at::kBFloat16)
      me_ok(me_pool_max_backward_bf16(ptr<uint16_t>(grad_out), c, ptr<int32_t>(tbl), km->n_in, km->volume,
                                      ptr<int32_t>(num_nonzero), ptr<uint16_t>(grad_in), stream_of(dev)));
    else
      me_ok(me_pool_max_backward_f32(ptr<float>(grad_out), c, ptr<int32_t>(tbl), km->n_in, km->volume,
                                     ptr<int32_t>(num_nonzero), ptr<float>(grad_in), stream_of(dev)));
    return grad_in;
  }
  const bool avg = pooling_mode == LOCAL_AVG;
  return pool_sum(grad_out, km->table("in"), km->n_in, km->volume, avg ? num_nonzero : Tensor(), false, false).first;
}

std::pair<Tensor, Tensor> local_pooling_transpose_forward(const Tensor &in_feat, const ivec &ks, const ivec &st,
                                                          const ivec &dl, int region_type, bool generate_new_coordinates,
                                                          int pooling_mode, CoordinateMapKey *in_key,
                                                          CoordinateMapKey *out_key, CoordinateMapManager *mgr,
                                                          const ivec &offsets) {
  (void)pooling_mode;
  check(!generate_new_coordinates, "generate_new_coordinates (stride_region) is not part of the hot path yet");
  prepare_pool(in_feat, st, in_key, out_key, mgr, true);
  auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, region_type, true, true, offsets);
  return pool_sum(in_feat, km->table("out"), km->n_out, km->volume, Tensor(), false, true);
}

Tensor local_pooling_transpose_backward(const Tensor &in_feat, Tensor grad_out, const Tensor &num_nonzero, const ivec &ks,
                                        const ivec &st, const ivec &dl, int region_type, int pooling_mode,
                                        CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr,
                                        const ivec &offsets) {
  (void)num_nonzero;
  (void)pooling_mode;
  grad_out = grad_out.contiguous();
  check_feat("grad_out_feat", grad_out);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, region_type, true, true, offsets);
  return pool_sum(grad_out, km->table("in"), km->n_in, km->volume, Tensor(), false, false).first;
}

// ---- channelwise (depthwise) convolution (csrc/conv_channelwise.hip; twin of backend.ChannelwiseConvolution*GPU) --------
static void check_cw(const Tensor &in_feat, const Tensor &kernel, const Tensor &bias, int64_t volume) {
  check_feat("in_feat", in_feat);
  check(in_feat.dim() == 2, "in_feat.dim() must be 2");
  check(kernel.is_cuda() && kernel.is_contiguous(), "kernel must be a contiguous CUDA (ROCm) tensor");
  const int64_t c = in_feat.size(1);
  check(kernel.dim() == 2 && kernel.size(0) == volume && kernel.size(1) == c,
        "kernel shape != (kernel volume, channels)");
  const at::ScalarType kt = in_feat.scalar_type() == at::kDouble ? at::kDouble : at::kFloat;
  check(kernel.scalar_type() == kt, "kernel must be float64 for float64 features and float32 otherwise");
  check(kernel.device() == in_feat.device(), "kernel and features must be on one device");
  if (bias.defined()) {
    check(bias.is_cuda() && bias.is_contiguous() && bias.numel() == c, "bias must be a contiguous CUDA tensor of C values");
    check(bias.scalar_type() == kernel.scalar_type(), "bias must have the kernel's dtype");
    check(bias.device() == in_feat.device(), "bias and features must be on one device");
  }
}

Tensor channelwise_forward(const Tensor &in_feat, const Tensor &kernel, const Tensor &bias, const ivec &ks,
                           const ivec &st, const ivec &dl, int region_type, CoordinateMapKey *in_key,
                           CoordinateMapKey *out_key, CoordinateMapManager *mgr, const ivec &offsets) {
  prepare_pool(in_feat, st, in_key, out_key, mgr, false);
  auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, region_type, false, false, offsets);
  check_cw(in_feat, kernel, bias, km->volume);
  const c10::Device dev = in_feat.device();
  const int c = (int)in_feat.size(1);
  Tensor out = at::empty({km->n_out, c}, in_feat.options());
  Tensor tbl = km->table("out");
  c10::DeviceGuard guard(dev);
  if (in_feat.scalar_type() == at::kDouble)
    me_ok(me_cwconv_forward_f64(ptr<double>(in_feat), c, ptr<double>(kernel), ptr<double>(bias), ptr<int32_t>(tbl),
                                km->n_in, km->n_out, km->volume, ptr<double>(out), stream_of(dev)));
  else if (in_feat.scalar_type() == at::kBFloat16)
    me_ok(me_cwconv_forward_bf16(ptr<uint16_t>(in_feat), c, ptr<float>(kernel), ptr<float>(bias), ptr<int32_t>(tbl),
                                 km->n_in, km->n_out, km->volume, ptr<uint16_t>(out), stream_of(dev)));
  else
    me_ok(me_cwconv_forward_f32(ptr<float>(in_feat), c, ptr<float>(kernel), ptr<float>(bias), ptr<int32_t>(tbl),
                                km->n_in, km->n_out, km->volume, ptr<float>(out), stream_of(dev)));
  return out;
}

std::tuple<Tensor, Tensor, Tensor> channelwise_backward(const Tensor &in_feat, Tensor grad_out, const Tensor &kernel,
                                                        const ivec &ks, const ivec &st, const ivec &dl, int region_type,
                                                        CoordinateMapKey *in_key, CoordinateMapKey *out_key,
                                                        CoordinateMapManager *mgr, bool need_grad_in,
                                                        bool need_grad_bias, const ivec &offsets) {
  check_feat("in_feat", in_feat);
  grad_out = grad_out.contiguous();
  check_feat("grad_out_feat", grad_out);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  check(grad_out.dim() == 2 && grad_out.size(1) == in_feat.size(1), "Output feature size and kernel size mismatch");
  auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, region_type, false, false, offsets);
  check_cw(in_feat, kernel, Tensor(), km->volume);
  check(in_feat.size(0) == km->n_in, "Invalid in_feat size");
  check(grad_out.size(0) == km->n_out, "Invalid grad_out size");
  const c10::Device dev = in_feat.device();
  const int c = (int)in_feat.size(1);
  Tensor grad_in = need_grad_in ? at::empty({km->n_in, c}, in_feat.options()) : Tensor();
  Tensor grad_kernel = at::empty({km->volume, c}, kernel.options());
  Tensor grad_bias = need_grad_bias ? at::empty({c}, kernel.options()) : Tensor();
  Tensor tbl = km->table("in");
  c10::DeviceGuard guard(dev);
  if (in_feat.scalar_type() == at::kDouble) {
    me_ok(me_cwconv_backward_f64(ptr<double>(in_feat), ptr<double>(grad_out), c, ptr<double>(kernel), ptr<int32_t>(tbl),
                                 km->n_in, km->n_out, km->volume, need_grad_in ? 1 : 0, ptr<double>(grad_in),
                                 ptr<double>(grad_kernel), ptr<double>(grad_bias), nullptr, 0, stream_of(dev)));
    return {grad_in, grad_kernel, grad_bias};
  }
  const int64_t ws_bytes = me_cwconv_backward_workspace_bytes(km->n_in, km->volume, c);
  Tensor ws = workspace(ws_bytes, dev);
  if (in_feat.scalar_type() == at::kBFloat16)
    me_ok(me_cwconv_backward_bf16(ptr<uint16_t>(in_feat), ptr<uint16_t>(grad_out), c, ptr<float>(kernel),
                                  ptr<int32_t>(tbl), km->n_in, km->n_out, km->volume, need_grad_in ? 1 : 0,
                                  ptr<uint16_t>(grad_in), ptr<float>(grad_kernel), ptr<float>(grad_bias), vptr(ws),
                                  ws.numel(), stream_of(dev)));
  else
    me_ok(me_cwconv_backward_f32(ptr<float>(in_feat), ptr<float>(grad_out), c, ptr<float>(kernel), ptr<int32_t>(tbl),
                                 km->n_in, km->n_out, km->volume, need_grad_in ? 1 : 0, ptr<float>(grad_in),
                                 ptr<float>(grad_kernel), ptr<float>(grad_bias), vptr(ws), ws.numel(), stream_of(dev)));
  return {grad_in, grad_kernel, grad_bias};
}

// mode 0 sum / 1 avg / 2 max over the rows of each origin row -> (out, argmax | undefined, count | undefined)
static std::tuple<Tensor, Tensor, Tensor> global_pool(const Tensor &src, const Tensor &src2, const Tensor &rows,
                                                      int64_t n_batch, int mode) {
  const c10::Device dev = src.device();
  const int64_t n = src.size(0);
  const int c = (int)src.size(1);
  if (src2.defined()) check(src2.scalar_type() == src.scalar_type(), "the second factor must have the dtype of the input features");
  const bool f64 = src.scalar_type() == at::kDouble;
  Tensor out = at::empty({n_batch, c}, at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev));
  Tensor arg, cnt;
  if (mode == 2) arg = empty_i32({n_batch, c}, dev);
  else cnt = at::empty({n_batch}, at::TensorOptions().dtype(at::kFloat).device(dev));
  if (f64) {
    c10::DeviceGuard guard(dev);
    me_ok(me_global_pool_f64(ptr<double>(src), ptr<double>(src2), c, ptr<int32_t>(rows), n, (int)n_batch, mode,
                             ptr<double>(out), ptr<int32_t>(arg), ptr<float>(cnt), stream_of(dev)));
    return {out, arg, cnt};
  }
  Tensor ws = workspace(me_global_pool_workspace_bytes(n, (int)n_batch, c), dev);
  {
    c10::DeviceGuard guard(dev);
    if (src.scalar_type() == at::kBFloat16)
      me_ok(me_global_pool_bf16(ptr<uint16_t>(src), ptr<uint16_t>(src2), c, ptr<int32_t>(rows), n, (int)n_batch, mode,
                                ptr<float>(out), ptr<int32_t>(arg), ptr<float>(cnt), vptr(ws), ws.numel(), stream_of(dev)));
    else
      me_ok(me_global_pool_f32(ptr<float>(src), ptr<float>(src2), c, ptr<int32_t>(rows), n, (int)n_batch, mode,
                               ptr<float>(out), ptr<int32_t>(arg), ptr<float>(cnt), vptr(ws), ws.numel(), stream_of(dev)));
  }
  if (src.scalar_type() != at::kFloat) out = out.to(src.scalar_type());
  return {out, arg, cnt};
}

std::pair<Tensor, Tensor> global_pooling_forward(const Tensor &in_feat, int pooling_mode, CoordinateMapKey *in_key,
                                                 CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
  check_feat("in_feat", in_feat);
  check(in_feat.dim() == 2, "Invalid in_feat.dim()");
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik) || mgr->exists_field(ik), "coordinate map not found");
  check(in_feat.size(0) == mgr->pool_size(ik, in_feat.size(0)), "Invalid in_feat size");
  const int m = global_mode(pooling_mode);
  // a field key (src/global_pooling_gpu.cu:58, 74-85): origin_field() and the field's row table; same kernels
  auto pr = mgr->pool_rows(ik, in_feat.size(0));
  if (!out_key->key_set) out_key->set_key(pr.second.first, pr.second.second);
  Tensor rows = pr.first;
  const int64_t n_batch = mgr->get(out_key->get())->n;
  auto r = global_pool(in_feat, Tensor(), rows, n_batch, m);
  return {std::get<0>(r), m == 2 ? std::get<1>(r) : std::get<2>(r)};
}

static Tensor broadcast(const Tensor &in_feat, const Tensor &glob, const Tensor &rows, int64_t n, int c, bool multiply) {
  const c10::Device dev = glob.device();
  if (in_feat.defined()) check(in_feat.scalar_type() == glob.scalar_type(), "in_feat must have the dtype of the input features");
  Tensor out = at::empty({n, c}, glob.options());
  c10::DeviceGuard guard(dev);
  if (glob.scalar_type() == at::kDouble)
    me_ok(me_broadcast_f64(ptr<double>(in_feat), ptr<double>(glob), ptr<int32_t>(rows), n, c, multiply ? 1 : 0,
                           ptr<double>(out), stream_of(dev)));
  else if (glob.scalar_type() == at::kBFloat16)
    me_ok(me_broadcast_bf16(ptr<uint16_t>(in_feat), ptr<uint16_t>(glob), ptr<int32_t>(rows), n, c, multiply ? 1 : 0,
                            ptr<uint16_t>(out), stream_of(dev)));
  else
    me_ok(me_broadcast_f32(ptr<float>(in_feat), ptr<float>(glob), ptr<int32_t>(rows), n, c, multiply ? 1 : 0,
                           ptr<float>(out), stream_of(dev)));
  return out;
}

Tensor global_pooling_backward(const Tensor &in_feat, Tensor grad_out, const Tensor &num_nonzero, int pooling_mode,
                               CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
  (void)out_key;
  check_feat("in_feat", in_feat);
  grad_out = grad_out.contiguous();
  check_feat("grad_out_feat", grad_out);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  const int m = global_mode(pooling_mode);
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  if (m == 2) {
    Tensor grad_in = at::zeros({n, c}, in_feat.options());
    Tensor flat = num_nonzero.reshape({-1});
    Tensor valid = flat.ge(0);
    grad_in.view({-1}).index_put_({flat.index({valid}).to(at::kLong)}, grad_out.reshape({-1}).index({valid}));
    return grad_in;
  }
  Tensor g = grad_out;
  if (m == 1)
    g = ((g.scalar_type() == at::kDouble ? g : g.to(at::kFloat)) / num_nonzero.clamp_min(1.0).unsqueeze(1))
            .to(in_feat.scalar_type()).contiguous();
  Tensor rows = mgr->pool_rows(in_key->get(), n).first;
  return broadcast(Tensor(), g, rows, n, c, false);
}

Tensor broadcast_forward(const Tensor &in_feat, const Tensor &in_feat_glob, int broadcast_mode, CoordinateMapKey *in_key,
                         CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
  check_feat("in_feat", in_feat);
  check_feat("in_feat_glob", in_feat_glob);
  check(in_feat_glob.scalar_type() == in_feat.scalar_type(), "in_feat_glob must have the dtype of the input features");
  check(in_feat.size(1) == in_feat_glob.size(1), "feature sizes must match");
  check(in_feat.size(0) == mgr->pool_size(in_key->get(), in_feat.size(0)), "Invalid in_feat size");
  Tensor rows = mgr->pool_rows(in_key->get(), in_feat.size(0)).first;   // (a field key: an extension of the reference)
  check(in_feat_glob.size(0) == mgr->get(glob_key->get())->n, "Invalid in_feat_glob size");
  return broadcast(in_feat, in_feat_glob, rows, in_feat.size(0), (int)in_feat.size(1), broadcast_mode == 1);
}

std::pair<Tensor, Tensor> broadcast_backward(const Tensor &in_feat, const Tensor &in_feat_glob, Tensor grad_out,
                                             int broadcast_mode, CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
                                             CoordinateMapManager *mgr) {
  (void)glob_key;
  check_feat("in_feat", in_feat);
  check_feat("in_feat_glob", in_feat_glob);
  grad_out = grad_out.contiguous();
  check_feat("grad_out_feat", grad_out);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  Tensor rows = mgr->pool_rows(in_key->get(), in_feat.size(0)).first;
  const int64_t n_batch = in_feat_glob.size(0);
  if (broadcast_mode == 0) {
    Tensor grad_glob = std::get<0>(global_pool(grad_out, Tensor(), rows, n_batch, 0));
    return {grad_out.clone(), grad_glob};
  }
  Tensor grad_in = broadcast(grad_out, in_feat_glob, rows, in_feat.size(0), (int)in_feat.size(1), true);
  Tensor grad_glob = std::get<0>(global_pool(grad_out, in_feat, rows, n_batch, 0));
  return {grad_in, grad_glob};
}

// ---- instance normalisation (csrc/instance_norm.hip; twin of backend.InstanceNorm{Forward,Backward}GPU) ------------------------
static void inorm_check_vec(const char *name, const Tensor &t, const Tensor &in_feat, int64_t numel) {
  const at::ScalarType want = in_feat.scalar_type() == at::kDouble ? at::kDouble : at::kFloat;
  check(!t.defined() || (t.is_cuda() && t.is_contiguous() && t.scalar_type() == want && t.numel() == numel &&
                         t.device() == in_feat.device()),
        std::string(name) + " must be a contiguous GPU tensor of the parameter dtype (float64 for float64 features, float32 "
                            "otherwise) with one value per (instance and) channel, on the device of the features");
}

// -> (batch_row, n_batch); an unset glob_key becomes the origin map, as global_pooling_forward does
static std::pair<Tensor, int64_t> inorm_prepare(const Tensor &in_feat, CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
                                                CoordinateMapManager *mgr) {
  check_feat("in_feat", in_feat);
  check(in_feat.dim() == 2 && in_feat.size(1) > 0, "Invalid in_feat shape");
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik), "coordinate map not found");
  check(in_feat.size(0) == mgr->get(ik)->n, "Invalid in_feat size");
  if (!glob_key->key_set) {
    KeyT ok = mgr->origin();
    glob_key->set_key(ok.first, ok.second);
  }
  Tensor rows = mgr->origin_rows(ik);
  return {rows, mgr->get(glob_key->get())->n};
}

// The shared opening of the norm backward operators (twin of backend._norm_backward_prepare): grad_out made contiguous and
// cast to the dtype of in_feat -> (batch_row, n_batch, grad_in, grad_weight, grad_bias), allocated, not yet written
static std::tuple<Tensor, int, Tensor, Tensor, Tensor> norm_backward_prepare(
    const Tensor &in_feat, Tensor &grad_out, CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
    CoordinateMapManager *mgr, bool need_grad_in, bool need_grad_weight, bool need_grad_bias) {
  auto pr = inorm_prepare(in_feat, in_key, glob_key, mgr);
  grad_out = grad_out.contiguous();
  check_feat("grad_out_feat", grad_out);
  if (grad_out.scalar_type() != in_feat.scalar_type()) grad_out = grad_out.to(in_feat.scalar_type());
  check(grad_out.sizes() == in_feat.sizes(), "grad_out_feat must have the shape of in_feat");
  const auto popt = at::TensorOptions().dtype(in_feat.scalar_type() == at::kDouble ? at::kDouble : at::kFloat)
                        .device(in_feat.device());
  const int64_t c = in_feat.size(1);
  return {pr.first, (int)pr.second, need_grad_in ? at::empty_like(in_feat) : Tensor(),
          need_grad_weight ? at::empty({c}, popt) : Tensor(), need_grad_bias ? at::empty({c}, popt) : Tensor()};
}

std::tuple<Tensor, Tensor, Tensor> instance_norm_forward(const Tensor &in_feat, const Tensor &weight, const Tensor &bias,
                                                         double eps, CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
                                                         CoordinateMapManager *mgr) {
  auto pr = inorm_prepare(in_feat, in_key, glob_key, mgr);
  const Tensor &rows = pr.first;
  const int n_batch = (int)pr.second;
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  inorm_check_vec("weight", weight, in_feat, c);
  inorm_check_vec("bias", bias, in_feat, c);
  const c10::Device dev = in_feat.device();
  const bool f64 = in_feat.scalar_type() == at::kDouble;
  const auto popt = at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev);
  Tensor mean = at::empty({n_batch, c}, popt), rstd = at::empty({n_batch, c}, popt);
  Tensor out = at::empty_like(in_feat);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_inorm_stats_f64(ptr<double>(in_feat), ptr<int32_t>(rows), n, n_batch, c, eps, ptr<double>(mean),
                             ptr<double>(rstd), stream_of(dev)));
    me_ok(me_inorm_apply_f64(ptr<double>(in_feat), ptr<int32_t>(rows), n, n_batch, c, ptr<double>(mean), ptr<double>(rstd),
                             ptr<double>(weight), ptr<double>(bias), ptr<double>(out), stream_of(dev)));
    return {out, mean, rstd};
  }
  const int bf = in_feat.scalar_type() == at::kBFloat16 ? 1 : 0;
  Tensor ws = workspace(me_inorm_workspace_bytes(n, n_batch, c), dev);
  me_ok(me_inorm_stats(in_feat.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, (float)eps, ptr<float>(mean),
                       ptr<float>(rstd), vptr(ws), ws.numel(), stream_of(dev)));
  me_ok(me_inorm_apply(in_feat.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, ptr<float>(mean), ptr<float>(rstd),
                       ptr<float>(weight), ptr<float>(bias), out.data_ptr(), stream_of(dev)));
  return {out, mean, rstd};
}

std::tuple<Tensor, Tensor, Tensor> instance_norm_backward(const Tensor &in_feat, Tensor grad_out, const Tensor &weight,
                                                          const Tensor &mean, const Tensor &rstd, CoordinateMapKey *in_key,
                                                          CoordinateMapKey *glob_key, CoordinateMapManager *mgr,
                                                          bool need_grad_in, bool need_grad_weight, bool need_grad_bias) {
  auto [rows, n_batch, grad_in, grad_weight, grad_bias] =
      norm_backward_prepare(in_feat, grad_out, in_key, glob_key, mgr, need_grad_in, need_grad_weight, need_grad_bias);
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  inorm_check_vec("weight", weight, in_feat, c);
  check(mean.defined() && rstd.defined(), "instance norm backward needs mean and rstd");
  inorm_check_vec("mean", mean, in_feat, (int64_t)n_batch * c);
  inorm_check_vec("rstd", rstd, in_feat, (int64_t)n_batch * c);
  const c10::Device dev = in_feat.device();
  const bool f64 = in_feat.scalar_type() == at::kDouble;
  if (n == 0) {
    if (grad_weight.defined()) grad_weight.zero_();
    if (grad_bias.defined()) grad_bias.zero_();
    return {grad_in, grad_weight, grad_bias};
  }
  Tensor ws = workspace(me_inorm_workspace_bytes(n, n_batch, c), dev);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_inorm_backward_f64(ptr<double>(in_feat), ptr<double>(grad_out), ptr<int32_t>(rows), n, n_batch, c,
                                ptr<double>(mean), ptr<double>(rstd), ptr<double>(weight), ptr<double>(grad_in),
                                ptr<double>(grad_weight), ptr<double>(grad_bias), vptr(ws), ws.numel(), stream_of(dev)));
  } else {
    const int bf = in_feat.scalar_type() == at::kBFloat16 ? 1 : 0;
    me_ok(me_inorm_backward(in_feat.data_ptr(), grad_out.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c,
                            ptr<float>(mean), ptr<float>(rstd), ptr<float>(weight), vptr(grad_in), ptr<float>(grad_weight),
                            ptr<float>(grad_bias), vptr(ws), ws.numel(), stream_of(dev)));
  }
  return {grad_in, grad_weight, grad_bias};
}

// ---- group normalisation (csrc/group_norm.hip; twin of backend.GroupNorm{Forward,Backward}GPU) ---------------------------------
static int gnorm_groups(int64_t num_groups, int c) {
  check(num_groups > 0 && c % num_groups == 0, "the channel count " + std::to_string(c) +
                                                   " must be a multiple of num_groups " + std::to_string(num_groups));
  return (int)num_groups;
}

std::tuple<Tensor, Tensor, Tensor> group_norm_forward(const Tensor &in_feat, int64_t num_groups, const Tensor &weight,
                                                      const Tensor &bias, double eps, CoordinateMapKey *in_key,
                                                      CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
  auto pr = inorm_prepare(in_feat, in_key, glob_key, mgr);
  const Tensor &rows = pr.first;
  const int n_batch = (int)pr.second;
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  const int groups = gnorm_groups(num_groups, c);
  inorm_check_vec("weight", weight, in_feat, c);
  inorm_check_vec("bias", bias, in_feat, c);
  const c10::Device dev = in_feat.device();
  const bool f64 = in_feat.scalar_type() == at::kDouble;
  const auto popt = at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev);
  Tensor mean = at::empty({n_batch, groups}, popt), rstd = at::empty({n_batch, groups}, popt);
  Tensor out = at::empty_like(in_feat);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_gnorm_stats_f64(ptr<double>(in_feat), ptr<int32_t>(rows), n, n_batch, c, groups, eps, ptr<double>(mean),
                             ptr<double>(rstd), stream_of(dev)));
    me_ok(me_gnorm_apply_f64(ptr<double>(in_feat), ptr<int32_t>(rows), n, n_batch, c, groups, ptr<double>(mean),
                             ptr<double>(rstd), ptr<double>(weight), ptr<double>(bias), ptr<double>(out), stream_of(dev)));
    return {out, mean, rstd};
  }
  const int bf = in_feat.scalar_type() == at::kBFloat16 ? 1 : 0;
  Tensor ws = workspace(me_gnorm_workspace_bytes(n, n_batch, c, groups), dev);
  me_ok(me_gnorm_stats(in_feat.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, groups, (float)eps, ptr<float>(mean),
                       ptr<float>(rstd), vptr(ws), ws.numel(), stream_of(dev)));
  me_ok(me_gnorm_apply(in_feat.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, groups, ptr<float>(mean),
                       ptr<float>(rstd), ptr<float>(weight), ptr<float>(bias), out.data_ptr(), stream_of(dev)));
  return {out, mean, rstd};
}

std::tuple<Tensor, Tensor, Tensor> group_norm_backward(const Tensor &in_feat, Tensor grad_out, int64_t num_groups,
                                                       const Tensor &weight, const Tensor &mean, const Tensor &rstd,
                                                       CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
                                                       CoordinateMapManager *mgr, bool need_grad_in,
                                                       bool need_grad_weight, bool need_grad_bias) {
  auto [rows, n_batch, grad_in, grad_weight, grad_bias] =
      norm_backward_prepare(in_feat, grad_out, in_key, glob_key, mgr, need_grad_in, need_grad_weight, need_grad_bias);
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  const int groups = gnorm_groups(num_groups, c);
  inorm_check_vec("weight", weight, in_feat, c);
  check(mean.defined() && rstd.defined(), "group norm backward needs mean and rstd");
  inorm_check_vec("mean", mean, in_feat, (int64_t)n_batch * groups);
  inorm_check_vec("rstd", rstd, in_feat, (int64_t)n_batch * groups);
  const c10::Device dev = in_feat.device();
  const bool f64 = in_feat.scalar_type() == at::kDouble;
  if (n == 0) {
    if (grad_weight.defined()) grad_weight.zero_();
    if (grad_bias.defined()) grad_bias.zero_();
    return {grad_in, grad_weight, grad_bias};
  }
  Tensor ws = workspace(me_gnorm_workspace_bytes(n, n_batch, c, groups), dev);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_gnorm_backward_f64(ptr<double>(in_feat), ptr<double>(grad_out), ptr<int32_t>(rows), n, n_batch, c, groups,
                                ptr<double>(mean), ptr<double>(rstd), ptr<double>(weight), ptr<double>(grad_in),
                                ptr<double>(grad_weight), ptr<double>(grad_bias), vptr(ws), ws.numel(), stream_of(dev)));
  } else {
    const int bf = in_feat.scalar_type() == at::kBFloat16 ? 1 : 0;
    me_ok(me_gnorm_backward(in_feat.data_ptr(), grad_out.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, groups,
                            ptr<float>(mean), ptr<float>(rstd), ptr<float>(weight), vptr(grad_in), ptr<float>(grad_weight),
                            ptr<float>(grad_bias), vptr(ws), ws.numel(), stream_of(dev)));
  }
  return {grad_in, grad_weight, grad_bias};
}

// ---- conditional group normalisation (csrc/group_norm.hip, k_gnc_*; twin of backend.ConditionalGroupNorm{Forward,Backward}GPU)
static void gnorm_cond_check_mod(const char *name, const Tensor &t, const Tensor &in_feat, int64_t n_batch, int64_t c) {
  const at::ScalarType want = in_feat.scalar_type() == at::kDouble ? at::kDouble : at::kFloat;
  check(!t.defined() || (t.is_cuda() && t.is_contiguous() && t.scalar_type() == want && t.dim() == 2 &&
                         t.size(0) == n_batch && t.size(1) == c && t.device() == in_feat.device()),
        std::string(name) + " must be a contiguous GPU tensor of the parameter dtype (float64 for float64 features, float32 "
                            "otherwise) of shape [" + std::to_string(n_batch) + ", " + std::to_string(c) +
                            "] (one row per instance), on the device of the features");
}

std::tuple<Tensor, Tensor, Tensor> cond_group_norm_forward(const Tensor &in_feat, int64_t num_groups, const Tensor &weight,
                                                           const Tensor &bias, const Tensor &scale, const Tensor &shift,
                                                           int act, double eps, CoordinateMapKey *in_key,
                                                           CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
  auto pr = inorm_prepare(in_feat, in_key, glob_key, mgr);
  const Tensor &rows = pr.first;
  const int n_batch = (int)pr.second;
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  const int groups = gnorm_groups(num_groups, c);
  inorm_check_vec("weight", weight, in_feat, c);
  inorm_check_vec("bias", bias, in_feat, c);
  gnorm_cond_check_mod("scale", scale, in_feat, n_batch, c);
  gnorm_cond_check_mod("shift", shift, in_feat, n_batch, c);
  const c10::Device dev = in_feat.device();
  const bool f64 = in_feat.scalar_type() == at::kDouble;
  const auto popt = at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev);
  Tensor out = at::empty_like(in_feat);
  if (n == 0) return {out, at::zeros({n_batch, groups}, popt), at::full({n_batch, groups}, 1.0 / std::sqrt(eps), popt)};
  Tensor mean = at::empty({n_batch, groups}, popt), rstd = at::empty({n_batch, groups}, popt);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_gnorm_stats_f64(ptr<double>(in_feat), ptr<int32_t>(rows), n, n_batch, c, groups, eps, ptr<double>(mean),
                             ptr<double>(rstd), stream_of(dev)));
    me_ok(me_gnorm_cond_apply_f64(ptr<double>(in_feat), ptr<int32_t>(rows), n, n_batch, c, groups, ptr<double>(mean),
                                  ptr<double>(rstd), ptr<double>(weight), ptr<double>(bias), ptr<double>(scale),
                                  ptr<double>(shift), act, ptr<double>(out), stream_of(dev)));
    return {out, mean, rstd};
  }
  const int bf = in_feat.scalar_type() == at::kBFloat16 ? 1 : 0;
  Tensor ws = workspace(me_gnorm_cond_workspace_bytes(n, n_batch, c, groups), dev);
  me_ok(me_gnorm_stats(in_feat.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, groups, (float)eps, ptr<float>(mean),
                       ptr<float>(rstd), vptr(ws), ws.numel(), stream_of(dev)));
  me_ok(me_gnorm_cond_apply(in_feat.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, groups, ptr<float>(mean),
                            ptr<float>(rstd), ptr<float>(weight), ptr<float>(bias), ptr<float>(scale), ptr<float>(shift),
                            act, out.data_ptr(), vptr(ws), ws.numel(), stream_of(dev)));
  return {out, mean, rstd};
}

std::vector<Tensor> cond_group_norm_backward(const Tensor &in_feat, Tensor grad_out, int64_t num_groups,
                                             const Tensor &weight, const Tensor &bias, const Tensor &scale,
                                             const Tensor &shift, int act, const Tensor &mean, const Tensor &rstd,
                                             CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
                                             CoordinateMapManager *mgr, bool need_grad_in, bool need_grad_weight,
                                             bool need_grad_bias, bool need_grad_scale, bool need_grad_shift) {
  auto [rows, n_batch, grad_in, grad_weight, grad_bias] =
      norm_backward_prepare(in_feat, grad_out, in_key, glob_key, mgr, need_grad_in, need_grad_weight, need_grad_bias);
  const int64_t n = in_feat.size(0);
  const int c = (int)in_feat.size(1);
  const int groups = gnorm_groups(num_groups, c);
  inorm_check_vec("weight", weight, in_feat, c);
  inorm_check_vec("bias", bias, in_feat, c);
  gnorm_cond_check_mod("scale", scale, in_feat, n_batch, c);
  gnorm_cond_check_mod("shift", shift, in_feat, n_batch, c);
  check(mean.defined() && rstd.defined(), "conditional group norm backward needs mean and rstd");
  inorm_check_vec("mean", mean, in_feat, (int64_t)n_batch * groups);
  inorm_check_vec("rstd", rstd, in_feat, (int64_t)n_batch * groups);
  const c10::Device dev = in_feat.device();
  const bool f64 = in_feat.scalar_type() == at::kDouble;
  const auto popt = at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev);
  Tensor grad_scale = need_grad_scale ? at::empty({n_batch, c}, popt) : Tensor();
  Tensor grad_shift = need_grad_shift ? at::empty({n_batch, c}, popt) : Tensor();
  if (n == 0) {
    for (Tensor *g : {&grad_weight, &grad_bias, &grad_scale, &grad_shift})
      if (g->defined()) g->zero_();
    return {grad_in, grad_weight, grad_bias, grad_scale, grad_shift};
  }
  Tensor ws = workspace(me_gnorm_cond_workspace_bytes(n, n_batch, c, groups), dev);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_gnorm_cond_backward_f64(ptr<double>(in_feat), ptr<double>(grad_out), ptr<int32_t>(rows), n, n_batch, c, groups,
                                     ptr<double>(mean), ptr<double>(rstd), ptr<double>(weight), ptr<double>(bias),
                                     ptr<double>(scale), ptr<double>(shift), act, ptr<double>(grad_in),
                                     ptr<double>(grad_weight), ptr<double>(grad_bias), ptr<double>(grad_scale),
                                     ptr<double>(grad_shift), vptr(ws), ws.numel(), stream_of(dev)));
  } else {
    const int bf = in_feat.scalar_type() == at::kBFloat16 ? 1 : 0;
    me_ok(me_gnorm_cond_backward(in_feat.data_ptr(), grad_out.data_ptr(), bf, ptr<int32_t>(rows), n, n_batch, c, groups,
                                 ptr<float>(mean), ptr<float>(rstd), ptr<float>(weight), ptr<float>(bias), ptr<float>(scale),
                                 ptr<float>(shift), act, vptr(grad_in), ptr<float>(grad_weight), ptr<float>(grad_bias),
                                 ptr<float>(grad_scale), ptr<float>(grad_shift), vptr(ws), ws.numel(), stream_of(dev)));
  }
  return {grad_in, grad_weight, grad_bias, grad_scale, grad_shift};
}

// ---- per-instance multi-head attention (csrc/attention.hip; twin of backend.Attention{Forward,Backward}GPU) ------------------
// a 2-D CUDA operand with a contiguous last dimension (any row stride >= its width); anything else is copied
static Tensor attn_rows(const char *name, Tensor t, const Tensor *ref = nullptr) {
  check(t.is_cuda(), std::string(name) + " must be CUDA (ROCm) — the MI355X path has no CPU implementation");
  check(t.dim() == 2 && t.size(1) > 0, std::string("Invalid ") + name + " shape");
  check(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kDouble,
        std::string(name) + " must be float32, bfloat16 or float64");
  if (ref)
    check(t.scalar_type() == ref->scalar_type() && t.device() == ref->device() && t.size(1) == ref->size(1),
          std::string(name) + " must have the dtype, device and channel count of q");
  if (t.size(0) > 1 ? (t.stride(1) != 1 || t.stride(0) < t.size(1)) : !t.is_contiguous()) t = t.contiguous();
  return t;
}
static int64_t attn_stride(const Tensor &t) { return t.size(0) > 1 ? t.stride(0) : t.size(1); }

// a row list of the attention kernels; blk_tab undefined: no block table, the workgroups walk seg_ptr
struct AttnList {
  Tensor seg_ptr, seg_rows, blk_tab;
};
struct AttnPrep {
  int heads, c, n_seg;
  AttnList q, kv;
};

// out and grad_out as row operands of q's dtype and shape; lse: the statistics of the forward pass, of shape `lse_shape`
static void attn_backward_operands(const Tensor &q, Tensor &out, Tensor &grad_out, const Tensor &lse,
                                   at::IntArrayRef lse_shape, const char *lse_name) {
  out = attn_rows("out", out, &q);
  grad_out = attn_rows("grad_out", grad_out.to(q.scalar_type()));
  check(out.sizes() == q.sizes() && grad_out.sizes() == q.sizes(), "out and grad_out must have the shape of q");
  check(lse.is_cuda() && lse.is_contiguous() &&
            lse.scalar_type() == (q.scalar_type() == at::kDouble ? at::kDouble : at::kFloat) && lse.sizes() == lse_shape,
        std::string("lse must be the contiguous ") + lse_name + " statistics of the forward pass");
}

// attention on row lists (me_attn_forward_tab): a query row attends to the key rows of its own segment; twin of
// backend._list_attn_forward
static std::pair<Tensor, Tensor> list_attn_forward(const Tensor &q, const Tensor &k, const Tensor &v, const AttnPrep &p,
                                                   double scale) {
  const c10::Device dev = q.device();
  const bool f64 = q.scalar_type() == at::kDouble;
  const int64_t n_q = q.size(0), n_kv = k.size(0);
  Tensor out = at::empty({n_q, p.c}, q.options());
  Tensor lse = at::empty({n_q, p.heads}, at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev));
  const int32_t *spq = ptr<int32_t>(p.q.seg_ptr), *srq = ptr<int32_t>(p.q.seg_rows), *tq = ptr<int32_t>(p.q.blk_tab);
  const int32_t *spk = ptr<int32_t>(p.kv.seg_ptr), *srk = ptr<int32_t>(p.kv.seg_rows), *tk = ptr<int32_t>(p.kv.blk_tab);
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_attn_forward_tab_f64(ptr<double>(q), ptr<double>(k), ptr<double>(v), attn_stride(q), attn_stride(k),
                                  attn_stride(v), spq, srq, spk, srk, tq, tk, n_q, n_kv, p.n_seg, p.c, p.heads, scale,
                                  ptr<double>(out), p.c, ptr<double>(lse), stream_of(dev)));
  } else {
    const int bf = q.scalar_type() == at::kBFloat16 ? 1 : 0;
    me_ok(me_attn_forward_tab(q.data_ptr(), k.data_ptr(), v.data_ptr(), bf, attn_stride(q), attn_stride(k), attn_stride(v),
                              spq, srq, spk, srk, tq, tk, n_q, n_kv, p.n_seg, p.c, p.heads, (float)scale, out.data_ptr(),
                              p.c, ptr<float>(lse), stream_of(dev)));
  }
  return {out, lse};
}

// The gradients of list_attn_forward (twin of backend._list_attn_backward); one that is not requested is neither allocated
// nor computed.  No kv_splits: me_attn_backward_tab; else the query slices of me_attn_backward_split.  zero_unlisted: kv
// rows may sit in no segment; where the dK / dV pass writes the listed rows only (one slice, float64) grad_k / grad_v start
// as zeros.
static std::vector<Tensor> list_attn_backward(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out,
                                              const Tensor &lse, const Tensor &grad_out, const AttnPrep &p, double scale,
                                              bool need_grad_q, bool need_grad_k, bool need_grad_v,
                                              std::optional<int64_t> kv_splits = std::nullopt,
                                              bool zero_unlisted = false) {
  if (!(need_grad_q || need_grad_k || need_grad_v)) return {Tensor(), Tensor(), Tensor()};
  const c10::Device dev = q.device();
  const bool f64 = q.scalar_type() == at::kDouble;
  const int64_t n_q = q.size(0), n_kv = k.size(0);
  const bool zero_kv = zero_unlisted && (kv_splits == 1 || f64);
  auto new_kv = [&]() { return zero_kv ? at::zeros({n_kv, p.c}, q.options()) : at::empty({n_kv, p.c}, q.options()); };
  Tensor grad_q = need_grad_q ? at::empty({n_q, p.c}, q.options()) : Tensor();
  Tensor grad_k = need_grad_k ? new_kv() : Tensor();
  Tensor grad_v = need_grad_v ? new_kv() : Tensor();
  const int32_t *spq = ptr<int32_t>(p.q.seg_ptr), *srq = ptr<int32_t>(p.q.seg_rows), *tq = ptr<int32_t>(p.q.blk_tab);
  const int32_t *spk = ptr<int32_t>(p.kv.seg_ptr), *srk = ptr<int32_t>(p.kv.seg_rows), *tk = ptr<int32_t>(p.kv.blk_tab);
  c10::DeviceGuard guard(dev);
#define ME_LIST_ATTN_BWD_ARGS(P, SCALE)                                                                                 \
  attn_stride(q), attn_stride(k), attn_stride(v), attn_stride(out), attn_stride(grad_out), spq, srq, spk, srk, tq, tk, \
      n_q, n_kv, p.n_seg, p.c, p.heads, SCALE, P(grad_q), p.c, P(grad_k), p.c, P(grad_v), p.c
  if (f64) {
    const double *qd = ptr<double>(q), *kd = ptr<double>(k), *vd = ptr<double>(v), *od = ptr<double>(out),
                 *ld = ptr<double>(lse), *gd = ptr<double>(grad_out);
    if (!kv_splits)
      me_ok(me_attn_backward_tab_f64(qd, kd, vd, od, ld, gd, ME_LIST_ATTN_BWD_ARGS(ptr<double>, scale),
                                     stream_of(dev)));
    else
      me_ok(me_attn_backward_split_f64(qd, kd, vd, od, ld, gd, ME_LIST_ATTN_BWD_ARGS(ptr<double>, scale),
                                       (int32_t)*kv_splits, stream_of(dev)));
  } else {
    const int bf = q.scalar_type() == at::kBFloat16 ? 1 : 0;
    if (!kv_splits) {
      Tensor ws = workspace(me_attn_workspace_bytes(n_q, n_kv, p.n_seg, p.heads), dev);
      me_ok(me_attn_backward_tab(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ptr<float>(lse),
                                 grad_out.data_ptr(), bf, ME_LIST_ATTN_BWD_ARGS(vptr, (float)scale), vptr(ws),
                                 ws.numel(), stream_of(dev)));
    } else {
      Tensor ws = workspace(me_attn_split_workspace_bytes(n_q, n_kv, p.n_seg, p.c, p.heads,
                                                          (int32_t)std::max<int64_t>(*kv_splits, 1)), dev);
      me_ok(me_attn_backward_split(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ptr<float>(lse),
                                   grad_out.data_ptr(), bf, ME_LIST_ATTN_BWD_ARGS(vptr, (float)scale), vptr(ws),
                                   ws.numel(), (int32_t)*kv_splits, stream_of(dev)));
    }
  }
#undef ME_LIST_ATTN_BWD_ARGS
  return {grad_q, grad_k, grad_v};
}

static AttnPrep attn_prepare(Tensor &q, Tensor &k, Tensor &v, int64_t num_heads, CoordinateMapKey *q_key,
                             CoordinateMapKey *kv_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
  q = attn_rows("q", q);
  k = attn_rows("k", k, &q);
  v = attn_rows("v", v, &q);
  const KeyT &qk = q_key->get(), &kk = kv_key->get();
  check(mgr->exists(qk) && mgr->exists(kk), "coordinate map not found");
  check(q.size(0) == mgr->get(qk)->n, "Invalid q size");
  check(k.size(0) == mgr->get(kk)->n && v.size(0) == k.size(0), "Invalid k / v size");
  const int64_t c = q.size(1);
  check(num_heads > 0 && c % num_heads == 0, "the channel count " + std::to_string(c) +
                                                 " must be a multiple of num_heads " + std::to_string(num_heads));
  if (!glob_key->key_set) {
    KeyT ok = mgr->origin();
    glob_key->set_key(ok.first, ok.second);
  }
  const auto &lq = mgr->instance_rows(qk), &lkv = mgr->instance_rows(kk);
  return {(int)num_heads, (int)c, (int)mgr->get(glob_key->get())->n, {lq.first, lq.second, Tensor()},
          {lkv.first, lkv.second, Tensor()}};
}

std::pair<Tensor, Tensor> attention_forward(Tensor q, Tensor k, Tensor v, int64_t num_heads, double scale,
                                            CoordinateMapKey *q_key, CoordinateMapKey *kv_key, CoordinateMapKey *glob_key,
                                            CoordinateMapManager *mgr) {
  const AttnPrep p = attn_prepare(q, k, v, num_heads, q_key, kv_key, glob_key, mgr);
  return list_attn_forward(q, k, v, p, scale);
}

std::vector<Tensor> attention_backward(Tensor q, Tensor k, Tensor v, Tensor out, const Tensor &lse, Tensor grad_out,
                                       int64_t num_heads, double scale, CoordinateMapKey *q_key, CoordinateMapKey *kv_key,
                                       CoordinateMapKey *glob_key, CoordinateMapManager *mgr, bool need_grad_q,
                                       bool need_grad_k, bool need_grad_v) {
  const AttnPrep p = attn_prepare(q, k, v, num_heads, q_key, kv_key, glob_key, mgr);
  attn_backward_operands(q, out, grad_out, lse, {q.size(0), (int64_t)p.heads}, "[n_q, heads]");
  return list_attn_backward(q, k, v, out, lse, grad_out, p, scale, need_grad_q, need_grad_k, need_grad_v);
}

// ---- cross-attention to a dense context (csrc/attention.hip, ABI 1.20; twin of backend.CrossAttention{Forward,Backward}GPU):
// q on a map, k / v [B, L, C] or [B * L, C] row views, context row j in the instance with the j-th smallest batch index ------
static AttnPrep cross_attn_prepare(Tensor &q, Tensor &k, Tensor &v, Tensor lengths, int64_t num_heads,
                                   CoordinateMapKey *q_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
  q = attn_rows("q", q);
  check((k.dim() == 2 || k.dim() == 3) && v.dim() == k.dim() && k.sizes().slice(0, k.dim() - 1) == v.sizes().slice(0, k.dim() - 1),
        "k and v must be [B, L, C] or [B * L, C] with the same leading shape");
  if (!glob_key->key_set) {
    KeyT ok = mgr->origin();
    glob_key->set_key(ok.first, ok.second);
  }
  const int64_t n_batch = mgr->get(glob_key->get())->n;
  if (k.dim() == 3) {
    check(k.size(0) == n_batch, "the context holds " + std::to_string(k.size(0)) + " instances, the coordinate manager " +
                                    std::to_string(n_batch));
    k = k.reshape({-1, k.size(2)});
    v = v.reshape({-1, v.size(2)});
  }
  k = attn_rows("k", k, &q);
  v = attn_rows("v", v, &q);
  const KeyT &qk = q_key->get();
  check(mgr->exists(qk), "coordinate map not found");
  check(q.size(0) == mgr->get(qk)->n, "Invalid q size");
  check(n_batch > 0 && k.size(0) % n_batch == 0 && k.size(0) >= n_batch,
        "the context rows " + std::to_string(k.size(0)) + " must be a positive multiple of the instances " +
            std::to_string(n_batch));
  const int64_t tokens = k.size(0) / n_batch, c = q.size(1);
  check(num_heads > 0 && c % num_heads == 0, "the channel count " + std::to_string(c) +
                                                 " must be a multiple of num_heads " + std::to_string(num_heads));
  if (lengths.defined()) {
    check(lengths.dim() == 1 && lengths.numel() == n_batch && at::isIntegralType(lengths.scalar_type(), false),
          "context_lengths must be an integer tensor with one length per instance");
    lengths = lengths.to(q.device(), at::kInt).contiguous();
  }
  const auto &lq = mgr->instance_rows(qk);
  const std::vector<Tensor> lkv = mgr->context_rows(n_batch, tokens, q.device(), lengths);
  return {(int)num_heads, (int)c, (int)n_batch, {lq.first, lq.second, Tensor()}, {lkv[0], lkv[1], lkv[2]}};
}

std::pair<Tensor, Tensor> cross_attention_forward(Tensor q, Tensor k, Tensor v, Tensor context_lengths, int64_t num_heads,
                                                  double scale, CoordinateMapKey *q_key, CoordinateMapKey *glob_key,
                                                  CoordinateMapManager *mgr) {
  const AttnPrep p = cross_attn_prepare(q, k, v, context_lengths, num_heads, q_key, glob_key, mgr);
  return list_attn_forward(q, k, v, p, scale);
}

std::vector<Tensor> cross_attention_backward(Tensor q, Tensor k, Tensor v, Tensor context_lengths, Tensor out,
                                             const Tensor &lse, Tensor grad_out, int64_t num_heads, double scale,
                                             CoordinateMapKey *q_key, CoordinateMapKey *glob_key,
                                             CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k,
                                             bool need_grad_v, int64_t kv_splits) {
  const AttnPrep p = cross_attn_prepare(q, k, v, context_lengths, num_heads, q_key, glob_key, mgr);
  attn_backward_operands(q, out, grad_out, lse, {q.size(0), (int64_t)p.heads}, "[n_q, heads]");
  if (kv_splits == 0) {   // the argument, else the environment, else the library's policy
    const char *env = std::getenv("ME_AMD_ATTN_KV_SPLITS");
    if (env && *env) kv_splits = std::atoll(env);
  }
  if (kv_splits == 0) kv_splits = me_attn_kv_splits(q.size(0), k.size(0), p.n_seg, p.c, p.heads);
  return list_attn_backward(q, k, v, out, lse, grad_out, p, scale, need_grad_q, need_grad_k, need_grad_v, kv_splits,
                            context_lengths.defined());
}

// ---- local attention over a kernel map (csrc/local_attention.hip; twin of backend.LocalAttention{Forward,Backward}GPU) ----
struct LattnPrep {
  int heads, c;
  std::shared_ptr<KernelMap> km;
};
static LattnPrep lattn_prepare(Tensor &q, Tensor &k, Tensor &v, Tensor &bias, int64_t num_heads, const ivec &ks,
                               const ivec &st, const ivec &dl, int region_type, CoordinateMapKey *q_key,
                               CoordinateMapKey *kv_key, CoordinateMapManager *mgr, const ivec &offsets) {
  q = attn_rows("q", q);
  k = attn_rows("k", k, &q);
  v = attn_rows("v", v, &q);
  const KeyT &qk = q_key->get(), &kk = kv_key->get();
  check(mgr->exists(qk) && mgr->exists(kk), "coordinate map not found");
  check(q.size(0) == mgr->get(qk)->n, "Invalid q size");
  check(k.size(0) == mgr->get(kk)->n && v.size(0) == k.size(0), "Invalid k / v size");
  const int64_t c = q.size(1);
  check(num_heads > 0 && c % num_heads == 0, "the channel count " + std::to_string(c) +
                                                 " must be a multiple of num_heads " + std::to_string(num_heads));
  LattnPrep p;
  p.heads = (int)num_heads;
  p.c = (int)c;
  p.km = mgr->kernel_map(kk, qk, ks, st, dl, region_type, false, true, offsets);
  check(p.km->n_out == q.size(0) && p.km->n_in == k.size(0), "the kernel map does not match q / k");
  if (bias.defined()) {
    check(bias.is_cuda() && bias.dim() == 2 && bias.size(0) == num_heads && bias.size(1) == p.km->volume,
          "rel_pos_bias must be a CUDA tensor of shape (num_heads, kernel volume)");
    bias = bias.detach().to(q.scalar_type() == at::kDouble ? at::kDouble : at::kFloat).contiguous();
  }
  return p;
}

std::pair<Tensor, Tensor> local_attention_forward(Tensor q, Tensor k, Tensor v, Tensor bias, int64_t num_heads,
                                                  double scale, const ivec &ks, const ivec &st, const ivec &dl,
                                                  int region_type, CoordinateMapKey *q_key, CoordinateMapKey *kv_key,
                                                  CoordinateMapManager *mgr, const ivec &offsets) {
  const LattnPrep p = lattn_prepare(q, k, v, bias, num_heads, ks, st, dl, region_type, q_key, kv_key, mgr, offsets);
  const c10::Device dev = q.device();
  const bool f64 = q.scalar_type() == at::kDouble;
  const int64_t n_out = p.km->n_out, n_in = p.km->n_in, volume = p.km->volume;
  Tensor out = at::empty({n_out, p.c}, q.options());
  // lse[0]: the log-sum-exp; lse[1]: the residual of its fp32 rounding (zeros in float64)
  const auto lse_opts = at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev);
  Tensor lse = f64 ? at::zeros({2, n_out, p.heads}, lse_opts) : at::empty({2, n_out, p.heads}, lse_opts);
  Tensor tbl = p.km->table("out");
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_local_attn_forward_f64(ptr<double>(q), ptr<double>(k), ptr<double>(v), attn_stride(q), attn_stride(k),
                                    attn_stride(v), ptr<int32_t>(tbl), n_out, n_in, volume, p.c, p.heads, scale,
                                    ptr<double>(bias), ptr<double>(out), p.c, ptr<double>(lse), stream_of(dev)));
  } else {
    const int bf = q.scalar_type() == at::kBFloat16 ? 1 : 0;
    me_ok(me_local_attn_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), bf, attn_stride(q), attn_stride(k),
                                attn_stride(v), ptr<int32_t>(tbl), n_out, n_in, volume, p.c, p.heads, (float)scale,
                                ptr<float>(bias), out.data_ptr(), p.c, ptr<float>(lse),
                                ptr<float>(lse) + n_out * p.heads, stream_of(dev)));
  }
  return {out, lse};
}

std::vector<Tensor> local_attention_backward(Tensor q, Tensor k, Tensor v, Tensor bias, Tensor out, const Tensor &lse,
                                             Tensor grad_out, int64_t num_heads, double scale, const ivec &ks,
                                             const ivec &st, const ivec &dl, int region_type, CoordinateMapKey *q_key,
                                             CoordinateMapKey *kv_key, CoordinateMapManager *mgr, const ivec &offsets,
                                             bool need_grad_q, bool need_grad_k, bool need_grad_v, bool need_grad_bias) {
  const LattnPrep p = lattn_prepare(q, k, v, bias, num_heads, ks, st, dl, region_type, q_key, kv_key, mgr, offsets);
  attn_backward_operands(q, out, grad_out, lse, {2, q.size(0), (int64_t)p.heads}, "[2, n_out, heads]");
  const c10::Device dev = q.device();
  const bool f64 = q.scalar_type() == at::kDouble;
  need_grad_bias = need_grad_bias && bias.defined();
  if (!(need_grad_q || need_grad_k || need_grad_v || need_grad_bias)) return {Tensor(), Tensor(), Tensor(), Tensor()};
  const int64_t n_out = p.km->n_out, n_in = p.km->n_in, volume = p.km->volume;
  Tensor grad_q = need_grad_q ? at::empty({n_out, p.c}, q.options()) : Tensor();
  Tensor grad_k = need_grad_k ? at::empty({n_in, p.c}, q.options()) : Tensor();
  Tensor grad_v = need_grad_v ? at::empty({n_in, p.c}, q.options()) : Tensor();
  Tensor grad_bias = need_grad_bias ? at::empty({(int64_t)p.heads, volume},
                                                at::TensorOptions().dtype(f64 ? at::kDouble : at::kFloat).device(dev))
                                    : Tensor();
  Tensor tbl_out = p.km->table("out"), tbl_in = p.km->table("in");
  c10::DeviceGuard guard(dev);
  if (f64) {
    me_ok(me_local_attn_backward_f64(ptr<double>(q), ptr<double>(k), ptr<double>(v), ptr<double>(out), ptr<double>(lse),
                                     ptr<double>(grad_out), attn_stride(q), attn_stride(k), attn_stride(v),
                                     attn_stride(out), attn_stride(grad_out), ptr<int32_t>(tbl_out), ptr<int32_t>(tbl_in),
                                     n_out, n_in, volume, p.c, p.heads, scale, ptr<double>(bias), ptr<double>(grad_q), p.c,
                                     ptr<double>(grad_k), p.c, ptr<double>(grad_v), p.c, ptr<double>(grad_bias),
                                     stream_of(dev)));
  } else {
    const int bf = q.scalar_type() == at::kBFloat16 ? 1 : 0;
    Tensor ws = workspace(me_local_attn_workspace_bytes(n_out, p.heads, volume, need_grad_bias ? 1 : 0), dev);
    me_ok(me_local_attn_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ptr<float>(lse),
                                 ptr<float>(lse) + n_out * p.heads, grad_out.data_ptr(), bf, attn_stride(q), attn_stride(k), attn_stride(v), attn_stride(out),
                                 attn_stride(grad_out), ptr<int32_t>(tbl_out), ptr<int32_t>(tbl_in), n_out, n_in, volume,
                                 p.c, p.heads, (float)scale, ptr<float>(bias), vptr(grad_q), p.c, vptr(grad_k), p.c,
                                 vptr(grad_v), p.c, ptr<float>(grad_bias), vptr(ws), ws.numel(), stream_of(dev)));
  }
  return {grad_q, grad_k, grad_v, grad_bias};
}

// ---- serialized patch attention (csrc/serial_attention.hip + the _tab entry points of csrc/attention.hip; twin of
// backend.SerializedAttention{Forward,Backward}GPU): q, k, v on ONE map, lists and block table from mgr->patch_rows -------
int serial_order_code(const std::string &order) {
  static const char *names[4] = {"z", "z_trans", "hilbert", "hilbert_trans"};
  for (int i = 0; i < 4; ++i)
    if (order == names[i]) return i;
  throw std::invalid_argument("order must be one of ('z', 'z_trans', 'hilbert', 'hilbert_trans'), not '" + order + "'");
}

static AttnPrep serial_attn_prepare(Tensor &q, Tensor &k, Tensor &v, int64_t num_heads, int64_t patch_size,
                                    const std::string &order, CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
  q = attn_rows("q", q);
  k = attn_rows("k", k, &q);
  v = attn_rows("v", v, &q);
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik), "coordinate map not found");
  const int64_t n = mgr->get(ik)->n;
  check(q.size(0) == n && k.size(0) == n && v.size(0) == n, "Invalid q / k / v size");
  const int64_t c = q.size(1);
  check(num_heads > 0 && c % num_heads == 0, "the channel count " + std::to_string(c) +
                                                 " must be a multiple of num_heads " + std::to_string(num_heads));
  const std::vector<Tensor> &l = mgr->patch_rows(ik, patch_size, serial_order_code(order));
  const AttnList lists{l[0], l[1], l[2]};
  return {(int)num_heads, (int)c, (int)l[0].numel() - 1, lists, lists};
}

std::pair<Tensor, Tensor> serialized_attention_forward(Tensor q, Tensor k, Tensor v, int64_t num_heads, double scale,
                                                       int64_t patch_size, const std::string &order,
                                                       CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
  const AttnPrep p = serial_attn_prepare(q, k, v, num_heads, patch_size, order, in_key, mgr);
  return list_attn_forward(q, k, v, p, scale);
}

std::vector<Tensor> serialized_attention_backward(Tensor q, Tensor k, Tensor v, Tensor out, const Tensor &lse,
                                                  Tensor grad_out, int64_t num_heads, double scale, int64_t patch_size,
                                                  const std::string &order, CoordinateMapKey *in_key,
                                                  CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k,
                                                  bool need_grad_v) {
  const AttnPrep p = serial_attn_prepare(q, k, v, num_heads, patch_size, order, in_key, mgr);
  attn_backward_operands(q, out, grad_out, lse, {q.size(0), (int64_t)p.heads}, "[n, heads]");
  return list_attn_backward(q, k, v, out, lse, grad_out, p, scale, need_grad_q, need_grad_k, need_grad_v);
}

// ---- shifted-window attention (csrc/serial_attention.hip, ABI 1.21 + the _tab entry points of csrc/attention.hip; twin of
// backend.WindowAttention{Forward,Backward}GPU): q, k, v on ONE map, lists and block table from mgr->window_rows ------------
// (window sizes, shifts reduced modulo them), one value per spatial axis each, from one value (all axes) or one per axis
std::pair<ivec, ivec> window_args(const ivec &window_size, const ivec &shift, int dimension) {
  auto per_axis = [&](const char *name, const ivec &v) {
    if ((int)v.size() == dimension) return v;
    if (v.size() == 1) return ivec((size_t)dimension, v[0]);
    throw std::invalid_argument(std::string(name) + " must be an int or one int per spatial axis (" +
                                std::to_string(dimension) + "), got " + std::to_string(v.size()) + " values");
  };
  ivec sizes = per_axis("window_size", window_size), shifts = per_axis("shift", shift);
  for (int a = 0; a < dimension; ++a) {
    if (sizes[a] < 1) throw std::invalid_argument("window_size must be at least 1, got " + std::to_string(sizes[a]));
    shifts[a] = (int32_t)((((int64_t)shifts[a] % sizes[a]) + sizes[a]) % sizes[a]);
  }
  return {sizes, shifts};
}

static AttnPrep window_attn_prepare(Tensor &q, Tensor &k, Tensor &v, int64_t num_heads, const ivec &window_size,
                                    const ivec &shift, CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
  q = attn_rows("q", q);
  k = attn_rows("k", k, &q);
  v = attn_rows("v", v, &q);
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik), "coordinate map not found");
  const int64_t n = mgr->get(ik)->n;
  check(q.size(0) == n && k.size(0) == n && v.size(0) == n, "Invalid q / k / v size");
  const int64_t c = q.size(1);
  check(num_heads > 0 && c % num_heads == 0, "the channel count " + std::to_string(c) +
                                                 " must be a multiple of num_heads " + std::to_string(num_heads));
  const std::vector<Tensor> &l = mgr->window_rows(ik, window_size, shift);
  const AttnList lists{l[0], l[1], l[2]};
  return {(int)num_heads, (int)c, (int)l[0].numel() - 1, lists, lists};
}

std::pair<Tensor, Tensor> window_attention_forward(Tensor q, Tensor k, Tensor v, int64_t num_heads, double scale,
                                                   const ivec &window_size, const ivec &shift, CoordinateMapKey *in_key,
                                                   CoordinateMapManager *mgr) {
  const AttnPrep p = window_attn_prepare(q, k, v, num_heads, window_size, shift, in_key, mgr);
  return list_attn_forward(q, k, v, p, scale);
}

std::vector<Tensor> window_attention_backward(Tensor q, Tensor k, Tensor v, Tensor out, const Tensor &lse, Tensor grad_out,
                                              int64_t num_heads, double scale, const ivec &window_size, const ivec &shift,
                                              CoordinateMapKey *in_key, CoordinateMapManager *mgr, bool need_grad_q,
                                              bool need_grad_k, bool need_grad_v) {
  const AttnPrep p = window_attn_prepare(q, k, v, num_heads, window_size, shift, in_key, mgr);
  attn_backward_operands(q, out, grad_out, lse, {q.size(0), (int64_t)p.heads}, "[n, heads]");
  return list_attn_backward(q, k, v, out, lse, grad_out, p, scale, need_grad_q, need_grad_k, need_grad_v);
}

// ---- rotary position embedding from voxel coordinates (csrc/rope.hip, ABI 1.22; twin of
// backend.RotaryEmbedding{Forward,Backward}GPU): the channel pairs of every head rotated by the angles of mgr->rope_table -----
// one unit >= 1 per spatial axis: the tensor stride for an empty `unit`, else one value (all axes) or one per axis
ivec rope_units(const ivec &unit, const ivec &tensor_stride, int dimension) {
  if (unit.empty()) return ivec(tensor_stride.begin(), tensor_stride.begin() + dimension);
  ivec units = unit.size() == 1 ? ivec((size_t)dimension, unit[0]) : unit;
  if ((int)units.size() != dimension)
    throw std::invalid_argument("unit must be None, an int or one int per spatial axis (" + std::to_string(dimension) +
                                "), got " + std::to_string(unit.size()) + " values");
  for (int32_t u : units)
    if (u < 1) throw std::invalid_argument("every unit must be at least 1, got " + std::to_string(u));
  return units;
}

static Tensor rope_apply(Tensor x, int64_t num_heads, double base, const ivec &unit, CoordinateMapKey *in_key,
                         CoordinateMapManager *mgr, int sign) {
  x = attn_rows("x", x);
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik), "coordinate map not found");
  const int64_t n = mgr->get(ik)->n, c = x.size(1);
  check(x.size(0) == n, "Invalid x size");
  check(num_heads > 0 && c % num_heads == 0, "the channel count " + std::to_string(c) +
                                                 " must be a multiple of num_heads " + std::to_string(num_heads));
  const int64_t d = c / num_heads;
  const at::ScalarType st = x.scalar_type();
  const Tensor &table = mgr->rope_table(ik, d, base, unit, st == at::kDouble);
  Tensor y = at::empty({n, c}, x.options());
  if (n == 0) return y;
  const c10::Device dev = x.device();
  c10::DeviceGuard guard(dev);
  me_ok(me_rope_apply(x.data_ptr(), attn_stride(x), y.data_ptr(), c, n, (int32_t)num_heads, (int32_t)d, table.data_ptr(),
                      sign, st == at::kFloat ? ME_ROPE_F32 : st == at::kBFloat16 ? ME_ROPE_BF16 : ME_ROPE_F64,
                      stream_of(dev)));
  return y;
}

Tensor rotary_embedding_forward(Tensor x, int64_t num_heads, double base, const ivec &unit, CoordinateMapKey *in_key,
                                CoordinateMapManager *mgr) {
  return rope_apply(x, num_heads, base, unit, in_key, mgr, 1);
}

Tensor rotary_embedding_backward(Tensor grad_out, int64_t num_heads, double base, const ivec &unit,
                                 CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
  return rope_apply(grad_out, num_heads, base, unit, in_key, mgr, -1);
}

// ---- pruning (src/pruning_cpu.cpp:40-150, src/pruning_gpu.cu) ------------------------------------------------------------------
Tensor pruning_forward(const Tensor &in_feat, const Tensor &keep, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
                       CoordinateMapManager *mgr) {
  check_feat("in_feat", in_feat);
  check(keep.scalar_type() == at::kBool || keep.scalar_type() == at::kByte, "keep must be a boolean tensor");
  check(in_feat.dim() == 2 && keep.dim() == 1, "in_feat.dim() must be 2, keep.dim() 1");
  check(in_feat.size(0) == keep.size(0), "Input feature size and keep size mismatch");
  const KeyT &ik = in_key->get();
  check(mgr->exists(ik), "coordinate map not found");
  check(in_feat.size(0) == mgr->get(ik)->n, "Invalid in_feat size");
  if (!out_key->key_set) {
    KeyT ok = mgr->prune(ik, keep);
    out_key->set_key(ok.first, ok.second);
  }
  Tensor rows = mgr->pruning_rows(ik, out_key->get());
  return in_feat.index_select(0, rows.to(at::kLong));
}

Tensor pruning_backward(const Tensor &grad_out, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
                        CoordinateMapManager *mgr) {
  check_feat("grad_out_feat", grad_out);
  Tensor rows = mgr->pruning_rows(in_key->get(), out_key->get());
  Tensor grad_in = at::zeros({mgr->get(in_key->get())->n, grad_out.size(1)}, grad_out.options());
  grad_in.index_copy_(0, rows.to(at::kLong), grad_out);
  return grad_in;
}

// ---- batch normalisation over feature rows (csrc/norm.hip) ----------------------------------------------------------------------
static void bn_check(const Tensor &x) {
  check(x.is_cuda() && x.is_contiguous() && x.dim() == 2, "batch norm input must be a contiguous GPU matrix");
  check(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "batch norm input must be float32 or bfloat16");
  check(x.size(0) > 0, "batch norm needs at least one row");
}

// The kernels read and write the running statistics as float32 [c] and the batch counter as int64 (norm.hip).  Buffers
// of another dtype / layout (after `model.bfloat16()` the running statistics are bf16: c floats written into a 2c-byte
// buffer would corrupt its neighbours) go through float32 temporaries that are copied back; a counter that is not an
// int64 GPU scalar is incremented by torch.
static bool bn_stat_ok(const Tensor &t, int c) {
  return !t.defined() || (t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == c);
}

static void bn_check_vec(const char *name, const Tensor &t, int c) {
  check(!t.defined() || (t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() == c),
        std::string(name) + " must be a contiguous float32 GPU vector of one value per channel");
}

std::pair<Tensor, Tensor> bn_stats(const Tensor &x, double eps, double momentum, const Tensor &running_mean_,
                                   const Tensor &running_var_, const Tensor &num_batches_tracked_) {
  bn_check(x);
  const c10::Device dev = x.device();
  const int64_t n = x.size(0);
  const int c = (int)x.size(1);
  check(running_mean_.defined() == running_var_.defined(), "running_mean and running_var: both or none");
  check(!running_mean_.defined() || (running_mean_.numel() == c && running_var_.numel() == c),
        "running statistics must hold one value per channel");
  const bool direct = bn_stat_ok(running_mean_, c) && bn_stat_ok(running_var_, c);
  Tensor running_mean = running_mean_, running_var = running_var_;
  if (!direct) {
    running_mean = running_mean_.to(dev, at::kFloat).contiguous().clone();
    running_var = running_var_.to(dev, at::kFloat).contiguous().clone();
  }
  Tensor num_batches_tracked = num_batches_tracked_;
  if (num_batches_tracked.defined() &&
      !(num_batches_tracked.is_cuda() && num_batches_tracked.scalar_type() == at::kLong && num_batches_tracked.numel() == 1)) {
    num_batches_tracked_.add_(1);
    num_batches_tracked = Tensor();
  }
  Tensor mean = at::empty({c}, at::TensorOptions().dtype(at::kFloat).device(dev));
  Tensor rstd = at::empty({c}, at::TensorOptions().dtype(at::kFloat).device(dev));
  c10::DeviceGuard guard(dev);
  Tensor part;
  int tile_rows = 0;
  if (bn_partials_take(x, part, tile_rows)) {   // the producing convolution already summed its tiles
    const int64_t tiles = part.size(1);
    me_ok(me_bn_stats_from_tiles(ptr<float>(part), ptr<float>(part) + tiles * c, n, c, tile_rows, (float)eps,
                                 (float)momentum, ptr<float>(mean), ptr<float>(rstd), ptr<float>(running_mean),
                                 ptr<float>(running_var), ptr<int64_t>(num_batches_tracked), stream_of(dev)));
  } else {
    Tensor ws = workspace(me_bn_workspace_bytes(n, c), dev);
    me_ok(me_bn_stats(x.data_ptr(), x.scalar_type() == at::kBFloat16 ? 1 : 0, n, c, (float)eps, (float)momentum,
                      ptr<float>(mean), ptr<float>(rstd), ptr<float>(running_mean), ptr<float>(running_var),
                      ptr<int64_t>(num_batches_tracked), vptr(ws), ws.numel(), stream_of(dev)));
  }
  if (!direct) {
    running_mean_.copy_(running_mean);
    running_var_.copy_(running_var);
  }
  return {mean, rstd};
}

Tensor bn_apply(const Tensor &x, const Tensor &mean, const Tensor &rstd, const Tensor &gamma, const Tensor &beta,
                bool relu, const Tensor &skip) {
  bn_check(x);
  const c10::Device dev = x.device();
  const int cc = (int)x.size(1);
  bn_check_vec("mean", mean, cc);
  bn_check_vec("rstd", rstd, cc);
  bn_check_vec("gamma", gamma, cc);
  bn_check_vec("beta", beta, cc);
  check(mean.defined() && rstd.defined(), "batch norm needs mean and rstd");
  Tensor y = at::empty_like(x);
  c10::DeviceGuard guard(dev);
  const int bf = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  if (skip.defined()) {
    check(skip.sizes() == x.sizes() && skip.scalar_type() == x.scalar_type() && skip.is_contiguous(),
          "residual branch must match x");
    me_ok(me_bn_apply_residual(x.data_ptr(), skip.data_ptr(), bf, x.size(0), (int)x.size(1), ptr<float>(mean),
                               ptr<float>(rstd), ptr<float>(gamma), ptr<float>(beta), relu ? 1 : 0, y.data_ptr(),
                               stream_of(dev)));
  } else {
    me_ok(me_bn_apply(x.data_ptr(), bf, x.size(0), (int)x.size(1), ptr<float>(mean), ptr<float>(rstd), ptr<float>(gamma),
                      ptr<float>(beta), relu ? 1 : 0, y.data_ptr(), stream_of(dev)));
  }
  return y;
}

std::tuple<Tensor, Tensor, Tensor, Tensor> bn_backward(const Tensor &x, Tensor dy, const Tensor &yout, const Tensor &mean,
                                                       const Tensor &rstd, const Tensor &gamma, const Tensor &beta,
                                                       bool relu, bool residual, bool need_dskip) {
  bn_check(x);
  const c10::Device dev = x.device();
  const int64_t n = x.size(0);
  const int c = (int)x.size(1);
  bn_check_vec("mean", mean, c);
  bn_check_vec("rstd", rstd, c);
  bn_check_vec("gamma", gamma, c);
  bn_check_vec("beta", beta, c);
  check(mean.defined() && rstd.defined(), "batch norm backward needs mean and rstd");
  if (dy.scalar_type() != x.scalar_type()) dy = dy.to(x.scalar_type());
  dy = dy.contiguous();
  Tensor dx = at::empty_like(x);
  Tensor gg = grad_destination(gamma, {(int64_t)c}), gb = grad_destination(beta, {(int64_t)c});
  if (!gg.defined()) gg = at::empty({c}, at::TensorOptions().dtype(at::kFloat).device(dev));
  if (!gb.defined()) gb = at::empty({c}, at::TensorOptions().dtype(at::kFloat).device(dev));
  Tensor ws = workspace(me_bn_workspace_bytes(n, c), dev);
  Tensor dskip;
  const int bf = x.scalar_type() == at::kBFloat16 ? 1 : 0;
  c10::DeviceGuard guard(dev);
  if (residual) {
    if (need_dskip && relu) dskip = at::empty_like(x);
    me_ok(me_bn_backward_residual(x.data_ptr(), dy.data_ptr(), vptr(yout), bf, n, c, ptr<float>(mean), ptr<float>(rstd),
                                  ptr<float>(gamma), ptr<float>(beta), relu ? 1 : 0, dx.data_ptr(), vptr(dskip),
                                  ptr<float>(gg), ptr<float>(gb), vptr(ws), ws.numel(), stream_of(dev)));
    if (need_dskip && !relu) dskip = dy;
  } else {
    me_ok(me_bn_backward(x.data_ptr(), dy.data_ptr(), bf, n, c, ptr<float>(mean), ptr<float>(rstd), ptr<float>(gamma),
                         ptr<float>(beta), relu ? 1 : 0, dx.data_ptr(), ptr<float>(gg), ptr<float>(gb), vptr(ws),
                         ws.numel(), stream_of(dev)));
  }
  return {dx, dskip, gg, gb};
}

// ---- dense <-> sparse conversion (csrc/dense.hip; twin of backend.Dense*GPU: the same C-ABI calls in the same order) -----------
typedef std::vector<int64_t> lvec;

static int64_t cells_of(const lvec &shape) {
  int64_t n = 1;
  for (int64_t s : shape) n *= s;
  return n;
}

static void check_index(const char *name, const Tensor &t, at::ScalarType dtype, const c10::Device &dev, int64_t numel) {
  check(!t.defined() || (t.is_cuda() && t.is_contiguous() && t.scalar_type() == dtype && t.device() == dev &&
                         t.numel() == numel),
        std::string(name) + " must be a contiguous GPU tensor of its index type on the device of the features, one value "
                            "per row (cell) or per cell (grid)");
}

int64_t dense_policy(int64_t n, int64_t n_cells, int64_t c, int64_t elem_bytes, bool to_box) {
  return me_dense_policy(n, n_cells, (int32_t)c, (int32_t)elem_bytes, to_box ? 1 : 0);
}

std::tuple<Tensor, Tensor, Tensor> dense_cell_index(const Tensor &coordinates, const ivec &min_coordinate,
                                                    const ivec &divisor, const lvec &shape, bool want_grid) {
  check(coordinates.dim() == 2 && coordinates.is_cuda() && coordinates.scalar_type() == at::kInt &&
            coordinates.is_contiguous(),
        "coordinates must be a contiguous int32 [N, D+1] GPU tensor");
  const int64_t n = coordinates.size(0), ncol = coordinates.size(1);
  check((int64_t)min_coordinate.size() == ncol - 1 && (int64_t)divisor.size() == ncol - 1 && (int64_t)shape.size() == ncol,
        "min_coordinate / divisor / shape must have D / D / D+1 values");
  const c10::Device dev = coordinates.device();
  const int64_t n_cells = cells_of(shape);
  Tensor cell = at::empty({n}, at::TensorOptions().dtype(at::kLong).device(dev));
  Tensor flag = empty_i32({1}, dev);
  Tensor grid = want_grid ? empty_i32({n_cells}, dev) : Tensor();
  c10::DeviceGuard guard(dev);
  me_ok(me_dense_cell_index(ptr<int32_t>(coordinates), n, (int32_t)ncol, min_coordinate.data(), divisor.data(),
                            shape.data(), ptr<int64_t>(cell), ptr<int32_t>(flag), stream_of(dev)));
  if (want_grid) me_ok(me_dense_grid(ptr<int64_t>(cell), n, n_cells, ptr<int32_t>(grid), stream_of(dev)));
  return {cell, grid, flag};
}

Tensor dense_grid(const Tensor &cell, int64_t n_cells) {
  check(cell.is_cuda() && cell.scalar_type() == at::kLong && cell.is_contiguous() && cell.dim() == 1,
        "cell must be a contiguous int64 GPU vector");
  const c10::Device dev = cell.device();
  Tensor grid = empty_i32({n_cells}, dev);
  c10::DeviceGuard guard(dev);
  me_ok(me_dense_grid(ptr<int64_t>(cell), cell.numel(), n_cells, ptr<int32_t>(grid), stream_of(dev)));
  return grid;
}

Tensor dense_rows_to_box(const Tensor &rows, const Tensor &cell, const Tensor &grid, int64_t outer, int64_t inner,
                         int64_t policy) {
  check_feat("rows", rows);
  check(rows.dim() == 2 && rows.size(1) > 0, "Invalid rows shape");
  const c10::Device dev = rows.device();
  const int64_t n = rows.size(0), c = rows.size(1);
  check_index("cell", cell, at::kLong, dev, n);
  check_index("grid", grid, at::kInt, dev, outer * inner);
  Tensor box = at::empty({outer, c, inner}, rows.options());
  c10::DeviceGuard guard(dev);
  ScopedTimer tm("dense_rows_to_box", 0.0, stream_of(dev));
  me_ok(me_dense_rows_to_box(rows.data_ptr(), (int32_t)rows.element_size(), ptr<int64_t>(cell), ptr<int32_t>(grid), n, outer,
                             (int32_t)c, inner, box.data_ptr(), (int32_t)policy, stream_of(dev)));
  return box;
}

Tensor dense_box_to_rows(const Tensor &box, const Tensor &cell, const Tensor &grid, int64_t n, int64_t outer, int64_t inner,
                         int64_t policy) {
  check_feat("box", box);
  const c10::Device dev = box.device();
  check(outer * inner > 0 && box.numel() > 0 && box.numel() % (outer * inner) == 0,
        "box must hold outer * C * inner elements");
  const int64_t c = box.numel() / (outer * inner);
  check_index("cell", cell, at::kLong, dev, n);
  check_index("grid", grid, at::kInt, dev, outer * inner);
  Tensor rows = at::empty({n, c}, box.options());
  c10::DeviceGuard guard(dev);
  ScopedTimer tm("dense_box_to_rows", 0.0, stream_of(dev));
  me_ok(me_dense_box_to_rows(box.data_ptr(), (int32_t)box.element_size(), ptr<int64_t>(cell), ptr<int32_t>(grid), n, outer,
                             (int32_t)c, inner, rows.data_ptr(), (int32_t)policy, stream_of(dev)));
  return rows;
}

std::pair<Tensor, Tensor> dense_occupied(const Tensor &box, int64_t outer, int64_t inner, const lvec &shape) {
  check_feat("box", box);
  const c10::Device dev = box.device();
  const int64_t n_cells = outer * inner, ncol = (int64_t)shape.size();
  check(n_cells == cells_of(shape), "shape must have outer * inner cells");
  const auto lopt = at::TensorOptions().dtype(at::kLong).device(dev);
  if (n_cells == 0 || box.numel() == 0) return {empty_i32({0, ncol}, dev), at::empty({0}, lopt)};
  check(box.numel() % n_cells == 0, "box must hold outer * C * inner elements");
  const int64_t c = box.numel() / n_cells;
  Tensor ws = workspace(me_dense_occupied_workspace_bytes(n_cells), dev);
  int64_t n = 0;
  c10::DeviceGuard guard(dev);
  me_ok(me_dense_occupied_count(box.data_ptr(), (int32_t)box.element_size(), outer, (int32_t)c, inner, vptr(ws), ws.numel(),
                                &n, stream_of(dev)));
  Tensor coords = empty_i32({n, ncol}, dev), cell = at::empty({n}, lopt);
  if (n > 0)
    me_ok(me_dense_occupied_fill(vptr(ws), ws.numel(), (int32_t)ncol, shape.data(), ptr<int32_t>(coords), ptr<int64_t>(cell),
                                 stream_of(dev)));
  return {coords, cell};
}

Tensor dense_coordinates(const lvec &shape, c10::Device dev) {
  check(dev.is_cuda(), "DenseCoordinatesGPU generates on the GPU");
  if (!dev.has_index()) dev = c10::Device(dev.type(), c10::hip::current_device());
  Tensor coords = empty_i32({cells_of(shape), (int64_t)shape.size()}, dev);
  c10::DeviceGuard guard(dev);
  me_ok(me_dense_all_coords((int32_t)shape.size(), shape.data(), ptr<int32_t>(coords), stream_of(dev)));
  return coords;
}

}  // namespace meh
