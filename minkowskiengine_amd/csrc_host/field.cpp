// Tensor fields in the native host layer: the manager's field methods (src/coordinate_map_manager.cpp:200-350) and the
// field operators over csrc/field.hip.  C++ twin of the tensor-field parts of backend.py: same C-ABI calls in the same
// order, so both hosts give the same bits.
#include "host.hpp"

namespace meh {

void preload_device(const c10::Device &dev);

namespace {
void check_feat_f(const char *name, const Tensor &t) {
  check(t.is_contiguous(), std::string(name) + " must be contiguous");
  check(t.is_cuda(), std::string(name) + " must be CUDA (ROCm) — the MI355X path has no CPU implementation");
  check(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kDouble,
        std::string(name) + " must be float32, bfloat16 or float64");
}
at::ScalarType acc_type(const Tensor &feat) { return feat.scalar_type() == at::kDouble ? at::kDouble : at::kFloat; }
at::TensorOptions i32(const c10::Device &dev) { return at::TensorOptions().dtype(at::kInt).device(dev); }
void check_range(const char *name, const Tensor &t, int64_t n) {
  if (t.numel() == 0) return;
  const int64_t lo = t.min().item<int64_t>(), hi = t.max().item<int64_t>();
  check(lo >= 0 && hi < n, std::string(name) + " out of range [0, " + std::to_string(n) + ")");
}
}  // namespace

KeyT CoordinateMapManager::insert_field(const Tensor &coordinates, const ivec &tensor_stride,
                                        const std::string &string_id) {
  check(coordinates.dim() == 2, "coordinates must be 2-D");
  check(coordinates.is_cuda(), "coordinates must be on the GPU (the MI355X path has no CPU map)");
  check(coordinates.is_floating_point(), "field coordinates must be floating point");
  check(coordinates.size(1) - 1 == (int64_t)tensor_stride.size(),
        "The coordinate dimension (coordinate_size - 1) must match the size of tensor stride");
  preload_device(coordinates.device());
  KeyT key(tensor_stride, string_id);
  for (int i = 0; fields.count(key); ++i) key = KeyT(tensor_stride, (string_id.empty() ? "" : string_id + "-") + "f" + std::to_string(i));
  fields[key] = coordinates.detach().to(at::kFloat).contiguous();
  field_order.push_back(key);
  return key;
}

const Tensor &CoordinateMapManager::field(const KeyT &k) const {
  auto it = fields.find(k);
  check(it != fields.end(), "coordinate field not found");
  return it->second;
}

std::tuple<KeyT, Tensor, Tensor> CoordinateMapManager::field_to_sparse_insert_and_map(const KeyT &field_key,
                                                                                     const ivec &ts,
                                                                                     const std::string &string_id) {
  const Tensor x = field(field_key);
  check(x.size(1) - 1 == (int64_t)ts.size(),
        "The coordinate dimension (coordinate_size - 1) must match the size of tensor stride");
  const c10::Device dev = x.device();
  const int64_t n = x.size(0);
  const int ncol = (int)x.size(1);
  Tensor q = at::empty({n > 0 ? n : 1, ncol}, i32(dev));
  {
    c10::DeviceGuard guard(dev);
    me_ok(me_field_quantize_f32(ptr<float>(x), n, ncol, ts.data(), ptr<int32_t>(q), stream_of(dev)));
  }
  InsertResult r = insert_coords(q.narrow(0, 0, n), ts);
  const KeyT key = register_map(ts, r.map, string_id);
  field_maps[{field_key, key}] = {r.unique_map, r.inverse_map};
  return {key, r.unique_map, r.inverse_map};
}

std::pair<Tensor, Tensor> CoordinateMapManager::field_to_sparse_map(const KeyT &field_key, const KeyT &sparse_key) {
  const Tensor x = field(field_key);
  auto smap = get(sparse_key);
  check(x.size(1) == (int64_t)sparse_key.first.size() + 1, "The coordinate dimension mismatch.");
  auto it = field_lookups.find({field_key, sparse_key});
  if (it != field_lookups.end()) return it->second;
  const c10::Device dev = x.device();
  const int64_t n = x.size(0);
  const int ncol = (int)x.size(1);
  Tensor srow = at::empty({n > 0 ? n : 1}, i32(dev)), frow = at::empty({n > 0 ? n : 1}, i32(dev));
  Tensor ws = workspace(me_field_lookup_workspace_bytes(n), dev);
  int64_t n_hit = 0;
  {
    c10::DeviceGuard guard(dev);
    me_ok(me_field_lookup_f32(ptr<float>(x), n, ncol, sparse_key.first.data(), ptr<uint64_t>(smap->table),
                              smap->capacity, ptr<int32_t>(smap->coords), ptr<int32_t>(srow), ptr<int32_t>(frow), &n_hit,
                              vptr(ws), ws.numel(), stream_of(dev)));
  }
  Tensor s64 = srow.narrow(0, 0, n_hit).to(at::kLong), f64 = frow.narrow(0, 0, n_hit).to(at::kLong);
  field_lookups[{field_key, sparse_key}] = {s64, f64};
  return {s64, f64};
}

// ---- origin map of fields (src/coordinate_map_manager.cpp:516-560, 923-960) ---------------------------------------------
KeyT CoordinateMapManager::origin_field(const KeyT *field_key) {
  check(field_key != nullptr || !field_order.empty(), "origin_field() needs at least one coordinate field");
  const Tensor x = field(field_key != nullptr ? *field_key : field_order.front());   // default: the oldest field
  KeyT okey(ivec((size_t)x.size(1) - 1, 0), "");
  if (!maps.count(okey)) {
    Tensor batches = std::get<0>(at::_unique(at::round(x.select(1, 0)).to(at::kInt), /*sorted=*/true));
    Tensor oc = at::zeros({batches.numel(), x.size(1)}, i32(x.device()));
    oc.select(1, 0).copy_(batches);
    InsertResult r = insert_coords(oc.contiguous(), okey.first);   // unique rows: insertion order = sorted order
    put(okey, r.map);
  }
  return okey;
}

Tensor CoordinateMapManager::origin_field_rows(const KeyT &field_key) {
  const Tensor x = field(field_key);
  const KeyT okey = origin_field(&field_key);
  auto it = origin_field_rows_cache.find(field_key);
  if (it != origin_field_rows_cache.end()) return it->second;
  auto omap = get(okey);
  const c10::Device dev = x.device();
  const int64_t n = x.size(0);
  Tensor rows = at::empty({n > 0 ? n : 1}, i32(dev));
  {
    c10::DeviceGuard guard(dev);
    me_ok(me_field_origin_rows_f32(ptr<float>(x), n, (int)x.size(1), ptr<uint64_t>(omap->table), omap->capacity,
                                   ptr<int32_t>(omap->coords), ptr<int32_t>(rows), stream_of(dev)));
  }
  rows = rows.narrow(0, 0, n);
  check(n == 0 || rows.ge(0).all().item<bool>(),
        "the origin map does not contain every batch index of this coordinate field");
  origin_field_rows_cache[field_key] = rows;
  return rows;
}

// a key may name a field and a sparse map at once (separate namespaces): the sparse map wins unless only the field has
// that many rows (backend._is_field_input)
bool CoordinateMapManager::is_field_input(const KeyT &k, int64_t n_rows) const {
  auto f = fields.find(k);
  if (f == fields.end()) return false;
  auto m = maps.find(k);
  if (m == maps.end()) return true;
  return f->second.size(0) == n_rows && m->second->n != n_rows;
}

std::pair<Tensor, KeyT> CoordinateMapManager::pool_rows(const KeyT &k, int64_t n_rows) {
  if (is_field_input(k, n_rows)) return {origin_field_rows(k), origin_field(&k)};
  return {origin_rows(k), origin()};
}

int64_t CoordinateMapManager::pool_size(const KeyT &k, int64_t n_rows) const {
  if (is_field_input(k, n_rows)) return field(k).size(0);
  return get(k)->n;
}

std::tuple<Tensor, Tensor, Tensor, Tensor> CoordinateMapManager::interpolation_map(const KeyT &in_key,
                                                                                   const Tensor &samples) {
  auto smap = get(in_key);
  const ivec &ts = in_key.first;
  check(samples.dim() == 2 && samples.size(1) == (int64_t)ts.size() + 1, "samples must be [N, D+1]");
  check(samples.is_cuda(), "samples must be on the GPU (the MI355X path has no CPU map)");
  check(samples.scalar_type() == at::kFloat || samples.scalar_type() == at::kDouble,
        "samples must be float32 or float64");
  const Tensor x = samples.detach().contiguous();
  const c10::Device dev = x.device();
  const int64_t n = x.size(0);
  const int ncol = (int)x.size(1);
  int64_t cap = n << (ncol - 1);
  if (cap < 1) cap = 1;
  Tensor in_map = at::empty({cap}, i32(dev)), out_map = at::empty({cap}, i32(dev));
  Tensor w = at::empty({cap}, x.options());
  Tensor rowptr = at::empty({n + 1}, i32(dev));
  Tensor ws = workspace(me_field_interp_workspace_bytes(n, ncol), dev);
  int64_t nnz = 0;
  {
    c10::DeviceGuard guard(dev);
    if (x.scalar_type() == at::kDouble)
      me_ok(me_field_interp_map_f64(ptr<double>(x), n, ncol, ts.data(), ptr<uint64_t>(smap->table), smap->capacity,
                                    ptr<int32_t>(smap->coords), ptr<int32_t>(in_map), ptr<int32_t>(out_map),
                                    ptr<double>(w), ptr<int32_t>(rowptr), &nnz, vptr(ws), ws.numel(), stream_of(dev)));
    else
      me_ok(me_field_interp_map_f32(ptr<float>(x), n, ncol, ts.data(), ptr<uint64_t>(smap->table), smap->capacity,
                                    ptr<int32_t>(smap->coords), ptr<int32_t>(in_map), ptr<int32_t>(out_map),
                                    ptr<float>(w), ptr<int32_t>(rowptr), &nnz, vptr(ws), ws.numel(), stream_of(dev)));
  }
  return {in_map.narrow(0, 0, nnz), out_map.narrow(0, 0, nnz), w.narrow(0, 0, nnz), rowptr};
}

// ---- operators ------------------------------------------------------------------------------------------------------
std::tuple<Tensor, Tensor, Tensor> csr_from_coo(const Tensor &keys_, int64_t n_rows, const Tensor &cols_,
                                                const Tensor &vals_) {
  check(keys_.is_cuda() && keys_.dim() == 1, "keys must be a 1-D CUDA tensor");
  const Tensor keys = keys_.to(at::kInt).contiguous();
  const c10::Device dev = keys.device();
  const int64_t nnz = keys.numel();
  Tensor cols, vals;
  if (cols_.defined()) {
    cols = cols_.to(dev, at::kInt).contiguous();
    check(cols.numel() == nnz, "cols and keys must have one entry each");
  }
  if (vals_.defined()) {
    vals = vals_.contiguous();
    check(vals.is_cuda() && vals.numel() == nnz && (vals.element_size() == 4 || vals.element_size() == 8),
          "vals: 4- or 8-byte values");
  }
  Tensor rowptr = at::empty({n_rows + 1}, i32(dev));
  Tensor cols_out = at::empty({nnz > 0 ? nnz : 1}, i32(dev));
  Tensor vals_out = vals.defined() ? at::empty({nnz > 0 ? nnz : 1}, vals.options()) : Tensor();
  Tensor ws = workspace(me_csr_from_coo_workspace_bytes(nnz), dev);
  {
    c10::DeviceGuard guard(dev);
    me_ok(me_csr_from_coo(ptr<int32_t>(keys), ptr<int32_t>(cols), vptr(vals),
                          vals.defined() ? (int32_t)vals.element_size() : 0, nnz, n_rows, ptr<int32_t>(rowptr),
                          ptr<int32_t>(cols_out), vptr(vals_out), vptr(ws), ws.numel(), stream_of(dev)));
  }
  return {rowptr, cols_out.narrow(0, 0, nnz), vals_out.defined() ? vals_out.narrow(0, 0, nnz) : Tensor()};
}

Tensor csr_gather(Tensor x, const Tensor &rowptr, const Tensor &col, const Tensor &w, const Tensor &scale) {
  x = x.contiguous();
  check_feat_f("x", x);
  check(x.dim() == 2, "x must be 2-D");
  const at::ScalarType a = acc_type(x);
  for (const Tensor *t : {&w, &scale})
    check(!t->defined() || (t->is_cuda() && t->scalar_type() == a && t->is_contiguous()),
          "weights and scales must be contiguous CUDA tensors of the accumulation dtype");
  const int64_t n_rows = rowptr.numel() - 1;
  const int c = (int)x.size(1);
  Tensor y = at::empty({n_rows, (int64_t)c}, x.options());
  if (n_rows == 0 || c == 0) return y.zero_();
  const c10::Device dev = x.device();
  c10::DeviceGuard guard(dev);
  if (x.scalar_type() == at::kDouble)
    me_ok(me_csr_gather_f64(ptr<double>(x), c, ptr<int32_t>(rowptr), ptr<int32_t>(col), ptr<double>(w),
                            ptr<double>(scale), n_rows, ptr<double>(y), stream_of(dev)));
  else if (x.scalar_type() == at::kBFloat16)
    me_ok(me_csr_gather_bf16(ptr<uint16_t>(x), c, ptr<int32_t>(rowptr), ptr<int32_t>(col), ptr<float>(w),
                             ptr<float>(scale), n_rows, ptr<uint16_t>(y), stream_of(dev)));
  else
    me_ok(me_csr_gather_f32(ptr<float>(x), c, ptr<int32_t>(rowptr), ptr<int32_t>(col), ptr<float>(w),
                            ptr<float>(scale), n_rows, ptr<float>(y), stream_of(dev)));
  return y;
}

std::vector<Tensor> interpolation_forward(const Tensor &in_feat, const Tensor &tfield, const KeyT &in_key,
                                          CoordinateMapManager *mgr) {
  auto r = mgr->interpolation_map(in_key, tfield);
  check(in_feat.size(0) == mgr->get(in_key)->n, "Invalid in_feat size");
  Tensor out = csr_gather(in_feat, std::get<3>(r), std::get<0>(r), std::get<2>(r).to(acc_type(in_feat)), Tensor());
  return {out, std::get<0>(r), std::get<1>(r), std::get<2>(r)};
}

Tensor interpolation_backward(const Tensor &grad_out, const Tensor &in_map, const Tensor &out_map, const Tensor &weights,
                              const KeyT &in_key, CoordinateMapManager *mgr) {
  const int64_t n_in = mgr->get(in_key)->n;
  auto t = csr_from_coo(in_map, n_in, out_map, weights.to(acc_type(grad_out)));
  return csr_gather(grad_out, std::get<0>(t), std::get<1>(t), std::get<2>(t), Tensor());
}

Tensor coo_spmm(const Tensor &rows, const Tensor &cols, const Tensor &vals, int64_t dim_i, int64_t dim_j,
                const Tensor &mat2) {
  check(mat2.dim() == 2 && mat2.size(0) == dim_j, "mat2 must be [dim_j, C]");
  check(rows.numel() == cols.numel() && rows.numel() == vals.numel(), "rows, cols and vals must have one entry each");
  check_range("rows", rows, dim_i);
  check_range("cols", cols, dim_j);
  auto t = csr_from_coo(rows, dim_i, cols, vals.to(acc_type(mat2)));
  return csr_gather(mat2, std::get<0>(t), std::get<1>(t), std::get<2>(t), Tensor());
}

std::vector<Tensor> coo_spmm_average(const Tensor &rows, const Tensor &cols, int64_t dim_i, int64_t dim_j,
                                     const Tensor &mat2) {
  check(mat2.dim() == 2 && mat2.size(0) == dim_j, "mat2 must be [dim_j, C]");
  check(rows.numel() == cols.numel(), "rows and cols must have one entry each");
  check_range("rows", rows, dim_i);
  check_range("cols", cols, dim_j);
  auto t = csr_from_coo(rows, dim_i, cols, Tensor());
  const Tensor &rowptr = std::get<0>(t);
  const Tensor cnt = rowptr.narrow(0, 1, dim_i) - rowptr.narrow(0, 0, dim_i);
  const Tensor count = cnt.to(acc_type(mat2));
  const Tensor scale = at::where(count.gt(0), 1.0 / count.clamp_min(1), at::zeros_like(count));
  Tensor out = csr_gather(mat2, rowptr, std::get<1>(t), Tensor(), scale);
  Tensor row_of = at::repeat_interleave(at::arange(dim_i, i32(rowptr.device())), cnt.to(at::kLong));
  return {out, row_of, std::get<1>(t), scale.index({row_of.to(at::kLong)})};
}

// ---- direct max pooling (csrc/direct_pool.hip) ------------------------------------------------------------------------
static void check_dpool_index(const char *name, const Tensor &t) {
  check(t.is_cuda(), std::string(name) + " must be a CUDA (ROCm) tensor — the MI355X path has no CPU implementation");
  check(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, std::string(name) + " must be int32 or int64");
}

std::pair<Tensor, Tensor> direct_max_pool_fw(const Tensor &in_map_, const Tensor &out_map_, Tensor in_feat,
                                             int64_t out_nrows, bool is_sorted) {
  check_dpool_index("in_map", in_map_);
  check_dpool_index("out_map", out_map_);
  check(in_map_.dim() == 1 && out_map_.dim() == 1 && in_map_.numel() == out_map_.numel(),
        "in_map and out_map must be 1-D tensors of equal length");
  check(in_map_.scalar_type() == out_map_.scalar_type(), "in_map and out_map must have the same dtype");
  in_feat = in_feat.contiguous();
  check_feat_f("in_feat", in_feat);
  check(in_feat.dim() == 2, "Invalid in_feat.dim()");
  const c10::Device dev = in_feat.device();
  check(in_map_.device() == dev && out_map_.device() == dev, "all inputs must be on the same device");
  const Tensor in_map = in_map_.contiguous(), out_map = out_map_.contiguous();
  check(out_nrows >= 0, "Invalid number of out nrows");
  const int64_t n_in = in_feat.size(0), nmap = in_map.numel();
  const int c = (int)in_feat.size(1);
  Tensor out = at::empty({out_nrows, (int64_t)c}, in_feat.options());
  Tensor mask = at::empty({out_nrows, (int64_t)c}, in_map.options());
  if (out_nrows == 0 || c == 0) {
    check(nmap == 0 || c == 0, "Invalid number of out nrows");
    return {out, mask};
  }
  Tensor ws = workspace(me_direct_max_pool_workspace_bytes(nmap, out_nrows), dev);
  const int ib = (int)in_map.element_size(), sorted = is_sorted ? 1 : 0;
  c10::DeviceGuard guard(dev);
  if (in_feat.scalar_type() == at::kDouble)
    me_ok(me_direct_max_pool_f64(ptr<double>(in_feat), c, vptr(in_map), vptr(out_map), ib, nmap, n_in, out_nrows, sorted,
                                 ptr<double>(out), vptr(mask), vptr(ws), ws.numel(), stream_of(dev)));
  else if (in_feat.scalar_type() == at::kBFloat16)
    me_ok(me_direct_max_pool_bf16(ptr<uint16_t>(in_feat), c, vptr(in_map), vptr(out_map), ib, nmap, n_in, out_nrows,
                                  sorted, ptr<uint16_t>(out), vptr(mask), vptr(ws), ws.numel(), stream_of(dev)));
  else
    me_ok(me_direct_max_pool_f32(ptr<float>(in_feat), c, vptr(in_map), vptr(out_map), ib, nmap, n_in, out_nrows, sorted,
                                 ptr<float>(out), vptr(mask), vptr(ws), ws.numel(), stream_of(dev)));
  return {out, mask};
}

Tensor direct_max_pool_bw(Tensor grad_out, const Tensor &max_index_, int64_t in_nrows) {
  check_dpool_index("max_index", max_index_);
  grad_out = grad_out.contiguous();
  check_feat_f("grad_out_feat", grad_out);
  check(grad_out.dim() == 2 && max_index_.sizes() == grad_out.sizes(), "max_index must have the shape of grad_out_feat");
  const c10::Device dev = grad_out.device();
  check(max_index_.device() == dev, "all inputs must be on the same device");
  const Tensor max_index = max_index_.contiguous();
  check(in_nrows >= 0, "Invalid number of in nrows");
  const int64_t n_out = grad_out.size(0);
  const int c = (int)grad_out.size(1);
  Tensor grad_in = at::empty({in_nrows, (int64_t)c}, grad_out.options());
  if (in_nrows == 0 || c == 0) return grad_in;
  Tensor ws = workspace(me_direct_max_pool_backward_workspace_bytes(n_out, c), dev);
  const int ib = (int)max_index.element_size();
  c10::DeviceGuard guard(dev);
  if (grad_out.scalar_type() == at::kDouble)
    me_ok(me_direct_max_pool_backward_f64(ptr<double>(grad_out), vptr(max_index), ib, n_out, c, in_nrows,
                                          ptr<double>(grad_in), vptr(ws), ws.numel(), stream_of(dev)));
  else if (grad_out.scalar_type() == at::kBFloat16)
    me_ok(me_direct_max_pool_backward_bf16(ptr<uint16_t>(grad_out), vptr(max_index), ib, n_out, c, in_nrows,
                                           ptr<uint16_t>(grad_in), vptr(ws), ws.numel(), stream_of(dev)));
  else
    me_ok(me_direct_max_pool_backward_f32(ptr<float>(grad_out), vptr(max_index), ib, n_out, c, in_nrows,
                                          ptr<float>(grad_in), vptr(ws), ws.numel(), stream_of(dev)));
  return grad_in;
}

// ---- arithmetic across coordinate maps (csrc/union_arith.hip) ----------------------------------------------------------
int union_arith_op(const std::string &op) {
  if (op == "add") return ME_UNION_ADD;
  if (op == "sub") return ME_UNION_SUB;
  if (op == "mul") return ME_UNION_MUL;
  check(op == "div", "op must be one of add, sub, mul, div");
  return ME_UNION_DIV;
}

static void check_union_table(const char *name, const Tensor &t, int64_t n, const c10::Device &dev) {
  check(t.defined() && t.is_cuda() && t.scalar_type() == at::kInt && t.dim() == 1 && t.is_contiguous(),
        std::string(name) + " must be a contiguous 1-D int32 CUDA (ROCm) tensor");
  check(t.numel() == n && t.device() == dev,
        std::string(name) + " must have " + std::to_string(n) + " rows on the device of the features");
}

Tensor union_arith_fw(Tensor a_feat, Tensor b_feat, const Tensor &a_of_u, const Tensor &b_of_u, const std::string &op) {
  const int code = union_arith_op(op);
  a_feat = a_feat.contiguous();
  b_feat = b_feat.contiguous();
  check_feat_f("a_feat", a_feat);
  check_feat_f("b_feat", b_feat);
  check(a_feat.dim() == 2 && b_feat.dim() == 2, "features must be 2-D");
  check(a_feat.size(1) == b_feat.size(1), "channel counts differ");
  check(a_feat.scalar_type() == b_feat.scalar_type(), "feature dtypes differ");
  const c10::Device dev = a_feat.device();
  check(b_feat.device() == dev, "all inputs must be on the same device");
  const int64_t nu = a_of_u.defined() ? a_of_u.numel() : 0;
  check_union_table("a_of_u", a_of_u, nu, dev);
  check_union_table("b_of_u", b_of_u, nu, dev);
  const int64_t na = a_feat.size(0), nb = b_feat.size(0);
  const int c = (int)a_feat.size(1);
  Tensor out = at::empty({nu, (int64_t)c}, a_feat.options());
  if (nu == 0 || c == 0) return out;
  c10::DeviceGuard guard(dev);
  if (a_feat.scalar_type() == at::kDouble)
    me_ok(me_union_arith_f64(ptr<double>(a_feat), ptr<double>(b_feat), c, ptr<int32_t>(a_of_u), ptr<int32_t>(b_of_u), na,
                             nb, nu, code, ptr<double>(out), stream_of(dev)));
  else if (a_feat.scalar_type() == at::kBFloat16)
    me_ok(me_union_arith_bf16(ptr<uint16_t>(a_feat), ptr<uint16_t>(b_feat), c, ptr<int32_t>(a_of_u), ptr<int32_t>(b_of_u),
                              na, nb, nu, code, ptr<uint16_t>(out), stream_of(dev)));
  else
    me_ok(me_union_arith_f32(ptr<float>(a_feat), ptr<float>(b_feat), c, ptr<int32_t>(a_of_u), ptr<int32_t>(b_of_u), na, nb,
                             nu, code, ptr<float>(out), stream_of(dev)));
  return out;
}

std::pair<Tensor, Tensor> union_arith_bw(Tensor grad_out, Tensor a_feat, Tensor b_feat, const Tensor &u_of_a,
                                         const Tensor &u_of_b, const Tensor &a_of_u, const Tensor &b_of_u,
                                         const std::string &op, bool need_grad_a, bool need_grad_b) {
  const int code = union_arith_op(op);
  grad_out = grad_out.contiguous();
  a_feat = a_feat.contiguous();
  b_feat = b_feat.contiguous();
  check_feat_f("grad_out", grad_out);
  check(grad_out.dim() == 2, "grad_out must be 2-D");
  for (const Tensor *t : {&a_feat, &b_feat}) {
    check_feat_f("a_feat / b_feat", *t);
    check(t->dim() == 2 && t->size(1) == grad_out.size(1) && t->scalar_type() == grad_out.scalar_type() &&
              t->device() == grad_out.device(),
          "a_feat and b_feat must match grad_out in channels, dtype and device");
  }
  const c10::Device dev = grad_out.device();
  const int64_t na = a_feat.size(0), nb = b_feat.size(0), nu = grad_out.size(0);
  const int c = (int)grad_out.size(1);
  check_union_table("u_of_a", u_of_a, na, dev);
  check_union_table("u_of_b", u_of_b, nb, dev);
  check_union_table("a_of_u", a_of_u, nu, dev);
  check_union_table("b_of_u", b_of_u, nu, dev);
  Tensor grad_a, grad_b;
  if (need_grad_a) grad_a = at::empty_like(a_feat);
  if (need_grad_b) grad_b = at::empty_like(b_feat);
  if (c == 0 || !(need_grad_a || need_grad_b)) return {grad_a, grad_b};
  c10::DeviceGuard guard(dev);
  if (grad_out.scalar_type() == at::kDouble)
    me_ok(me_union_arith_backward_f64(ptr<double>(grad_out), ptr<double>(a_feat), ptr<double>(b_feat), c,
                                      ptr<int32_t>(u_of_a), ptr<int32_t>(u_of_b), ptr<int32_t>(a_of_u), ptr<int32_t>(b_of_u),
                                      na, nb, nu, code, ptr<double>(grad_a), ptr<double>(grad_b), stream_of(dev)));
  else if (grad_out.scalar_type() == at::kBFloat16)
    me_ok(me_union_arith_backward_bf16(ptr<uint16_t>(grad_out), ptr<uint16_t>(a_feat), ptr<uint16_t>(b_feat), c,
                                       ptr<int32_t>(u_of_a), ptr<int32_t>(u_of_b), ptr<int32_t>(a_of_u),
                                       ptr<int32_t>(b_of_u), na, nb, nu, code, ptr<uint16_t>(grad_a), ptr<uint16_t>(grad_b),
                                       stream_of(dev)));
  else
    me_ok(me_union_arith_backward_f32(ptr<float>(grad_out), ptr<float>(a_feat), ptr<float>(b_feat), c, ptr<int32_t>(u_of_a),
                                      ptr<int32_t>(u_of_b), ptr<int32_t>(a_of_u), ptr<int32_t>(b_of_u), na, nb, nu, code,
                                      ptr<float>(grad_a), ptr<float>(grad_b), stream_of(dev)));
  return {grad_a, grad_b};
}

}  // namespace meh
