// Local attention over a kernel map for gfx950 (MI355X): every row of the out map attends to the rows of the in map
// inside the kernel region around it (MinkowskiLocalSelfAttention, MinkowskiFunctional.local_attention; ABI 1.18).
//
//   s_ik = scale * <q[i, h, :], k[j, h, :]> + rel_pos_bias[h, k]      for the offsets k with j = nbr[k][i] >= 0
//   out[i, h, :] = sum_k softmax_k(s_ik) v[j, h, :],   lse[i, h] = log sum_k exp(s_ik)
//
// Local pooling whose weights are a softmax (csrc/pool.hip): the kernels are TARGET-stationary on the dense neighbour
// tables of the kernel map (nbr[k][out row] -> in row or -1, and its transpose), walk the offsets in ascending k and
// write every result row once: no atomics, a fixed summation order, bitwise reproducible gradients.  These are GATHER
// kernels, not MFMA kernels: every query has its own K keys, so there is no operand reuse for the matrix pipe.
//
// Work item = one (target row, head); its d channels lie on G = d / V adjacent lanes (V = the elements of a 16-byte piece:
// 8 bf16, 4 fp32), items are ordered with the head fastest, so the lanes of a row read one contiguous row.  A dot product
// is V fmas per lane and an xor butterfly over the G lanes (every lane ends with the same bits).  The walk over k is an
// online softmax (running maximum, sum, rescale): no per-K storage.  The index of offset k + 2 and the rows of offset
// k + 1 are loaded before the arithmetic of offset k.  A hole (-1) is read through the clamped index and masked by
// SELECTION: its score is -inf before the running maximum, its probability 0, and nothing gathered through it is ever
// multiplied (no 0 * Inf; no branch round a load, docs/HISTORY 10.5).  Scores, softmax and sums are fp32 for fp32 and
// bf16 rows, p is not rounded, one rounding at the store.
//
//   k_lattn_fwd      out-stationary: out, lse and lse_lo, the residual of the fp32 rounding of lse = m + log l, which the
//                    backward kernels subtract too: exp((s - lse) - lse_lo) adds up to 1 over a row however large |s| is
//   k_lattn_bwd_q    out-stationary: delta[i, h] = <dout_i, out_i> (workspace), dq, and per-workgroup sums of
//                    ds_ik = p_ik (dp_ik - delta_i) per (h, k) for the gradient of the bias
//   k_lattn_bias_merge   adds the workgroup sums in ascending workgroup order
//   k_lattn_bwd_kv   in-stationary on the transposed table: dk, dv
// delta and dp are the same chain of operations on the same lanes (lattn_dot), so a row with one neighbour (p = 1,
// out = v_j bitwise) has dp - delta == 0 and ds == 0 exactly — the rule of k_attn_delta (csrc/attention.hip).
// float64 twins: plain double, one thread per (row, head), any head dimension.
#include "piece.hpp"

#include <cmath>

namespace me {

constexpr int kLattnThreads = 256;
constexpr int kLattnBiasChunk = 8;   // offsets whose ds wait in LDS for one workgroup sum
constexpr int kLattnMinItems = 8;    // the fewest items of a workgroup: fp32, d = 128 (32 lanes an item)

template <int V>
__device__ __forceinline__ float lattn_dot_lane(const Piece<V> &a, const Piece<V> &b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) s = fmaf(a.v[j], b.v[j], s);
  return s;
}
// the sum over the G lanes of an item: an xor butterfly, commutative at every step, so every lane holds the same bits
template <int G>
__device__ __forceinline__ float lattn_group_sum(float x) {
#pragma unroll
  for (int m = 1; m < G; m <<= 1) x += __shfl_xor(x, m, 64);
  return x;
}
template <int V, int G>
__device__ __forceinline__ float lattn_dot(const Piece<V> &a, const Piece<V> &b) {
  return lattn_group_sum<G>(lattn_dot_lane<V>(a, b));
}
__device__ __forceinline__ float lattn_score(float scale, float dot, float bias) { return fmaf(scale, dot, bias); }

// (item, lane of the item) of a thread; the items past the end are clamped to the last one (the lanes of a wave stay
// together for the shuffles and the barriers) and `live` masks their stores
template <int G>
__device__ __forceinline__ bool lattn_item(int64_t n_items, int64_t &item, int &sub) {
  const int64_t gid = (int64_t)blockIdx.x * kLattnThreads + threadIdx.x;
  item = gid / G;
  sub = (int)(gid % G);
  const bool live = item < n_items;
  if (!live) item = n_items - 1;
  return live;
}

template <typename T, int D>
__global__ __launch_bounds__(kLattnThreads) void k_lattn_fwd(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int32_t *__restrict__ nbr, int64_t n_out, int volume, int heads, float scale,
    const float *__restrict__ bias, T *__restrict__ out, int64_t out_stride, float *__restrict__ lse,
    float *__restrict__ lse_lo) {
  constexpr int V = 16 / (int)sizeof(T), G = D / V;
  int64_t item;
  int sub;
  const bool live = lattn_item<G>(n_out * heads, item, sub);
  const int64_t row = item / heads;
  const int head = (int)(item - row * heads);
  const int ch = head * D + sub * V;
  const Piece<V> qv = load_piece<T, V>(q + row * q_stride + ch);
  const float *bh = bias ? bias + (int64_t)head * volume : nullptr;
  const int32_t *col = nbr + row;
  int32_t j0 = col[0];
  int32_t j1 = col[(int64_t)min(1, volume - 1) * n_out];
  int64_t jc = max(j0, 0);
  Piece<V> kv = load_piece<T, V>(k + jc * k_stride + ch);
  Piece<V> vv = load_piece<T, V>(v + jc * v_stride + ch);
  float m = -INFINITY, l = 0.f;
  Piece<V> acc;
#pragma unroll
  for (int j = 0; j < V; ++j) acc.v[j] = 0.f;
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t j2 = col[(int64_t)min(kk + 2, volume - 1) * n_out];
    jc = max(j1, 0);
    const Piece<V> kn = load_piece<T, V>(k + jc * k_stride + ch);
    const Piece<V> vn = load_piece<T, V>(v + jc * v_stride + ch);
    const bool has = j0 >= 0;
    const float dot = lattn_dot<V, G>(qv, kv);
    const float s = has ? lattn_score(scale, dot, bh ? bh[kk] : 0.f) : -INFINITY;
    const float mn = fmaxf(m, s);
    const float alpha = has ? expf(m - mn) : 1.f;
    const float p = has ? expf(s - mn) : 0.f;
    l = has ? fmaf(l, alpha, p) : l;
#pragma unroll
    for (int j = 0; j < V; ++j) acc.v[j] = has ? fmaf(p, vv.v[j], acc.v[j] * alpha) : acc.v[j];
    m = has ? mn : m;
    j0 = j1;
    j1 = j2;
    kv = kn;
    vv = vn;
  }
  if (!live) return;
  Piece<V> o;
#pragma unroll
  for (int j = 0; j < V; ++j) o.v[j] = l > 0.f ? acc.v[j] / l : 0.f;
  store_piece<T, V>(out + row * out_stride + ch, o);
  if (sub == 0) {
    // lse = m + log l rounds at ulp(|m|); its residual goes out too, so the backward pass sees the normaliser of THIS
    // softmax (the weights of a row then add up to 1 as in the forward pass, however large the scores)
    const float logl = logf(l), hi = m + logl;
    lse[item] = l > 0.f ? hi : -INFINITY;
    if (lse_lo != nullptr) lse_lo[item] = l > 0.f ? (m - hi) + logl : 0.f;
  }
}

template <typename T, int D>
__global__ __launch_bounds__(kLattnThreads) void k_lattn_bwd_q(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ out,
    const T *__restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride,
    int64_t dout_stride, const int32_t *__restrict__ nbr, int64_t n_out, int volume, int heads, float scale,
    const float *__restrict__ bias, const float *__restrict__ lse, const float *__restrict__ lse_lo,
    float *__restrict__ delta_out, T *__restrict__ dq,
    int64_t dq_stride, float *__restrict__ bias_part) {
  constexpr int V = 16 / (int)sizeof(T), G = D / V, IPW = kLattnThreads / G;
  __shared__ float s_ds[kLattnBiasChunk][IPW];
  int64_t item;
  int sub;
  const bool live = lattn_item<G>(n_out * heads, item, sub);
  const int64_t row = item / heads;
  const int head = (int)(item - row * heads);
  const int ch = head * D + sub * V;
  const Piece<V> gv = load_piece<T, V>(dout + row * dout_stride + ch);
  const Piece<V> ov = load_piece<T, V>(out + row * out_stride + ch);
  const float delta = lattn_dot<V, G>(gv, ov);
  if (live && sub == 0) delta_out[item] = delta;
  if (dq == nullptr && bias_part == nullptr) return;   // the same for every thread: only delta was wanted
  const Piece<V> qv = load_piece<T, V>(q + row * q_stride + ch);
  const float ls = lse[item], lo = lse_lo ? lse_lo[item] : 0.f;
  const float *bh = bias ? bias + (int64_t)head * volume : nullptr;
  const int32_t *col = nbr + row;
  int32_t j0 = col[0];
  int32_t j1 = col[(int64_t)min(1, volume - 1) * n_out];
  int64_t jc = max(j0, 0);
  Piece<V> kv = load_piece<T, V>(k + jc * k_stride + ch);
  Piece<V> vv = load_piece<T, V>(v + jc * v_stride + ch);
  Piece<V> acc;
#pragma unroll
  for (int j = 0; j < V; ++j) acc.v[j] = 0.f;
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t j2 = col[(int64_t)min(kk + 2, volume - 1) * n_out];
    jc = max(j1, 0);
    const Piece<V> kn = load_piece<T, V>(k + jc * k_stride + ch);
    const Piece<V> vn = load_piece<T, V>(v + jc * v_stride + ch);
    const bool has = j0 >= 0;
    const float dot = lattn_dot<V, G>(qv, kv);
    const float dp = lattn_dot<V, G>(gv, vv);
    const float s = lattn_score(scale, dot, bh ? bh[kk] : 0.f);
    const float p = has ? expf((s - ls) - lo) : 0.f;
    const float ds = has ? p * (dp - delta) : 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) acc.v[j] = has ? fmaf(ds, kv.v[j], acc.v[j]) : acc.v[j];
    if (bias_part != nullptr) {   // the same for every thread
      const int kq = kk % kLattnBiasChunk;
      if (sub == 0) s_ds[kq][threadIdx.x / G] = live ? ds : 0.f;
      if (kq == kLattnBiasChunk - 1 || kk == volume - 1) {
        // the sums of this workgroup over its items of every head, in ascending item order, for the offsets of the chunk
        __syncthreads();
        const int h0 = (int)(((int64_t)blockIdx.x * IPW) % heads);
        for (int idx = threadIdx.x; idx < (kq + 1) * heads; idx += kLattnThreads) {
          const int kc = idx / heads, h = idx - kc * heads;
          float sum = 0.f;
          for (int t = h - h0 + (h < h0 ? heads : 0); t < IPW; t += heads) sum += s_ds[kc][t];
          bias_part[((int64_t)blockIdx.x * heads + h) * volume + (kk - kq + kc)] = sum;
        }
        __syncthreads();
      }
    }
    j0 = j1;
    j1 = j2;
    kv = kn;
    vv = vn;
  }
  if (!live || dq == nullptr) return;
#pragma unroll
  for (int j = 0; j < V; ++j) acc.v[j] *= scale;
  store_piece<T, V>(dq + row * dq_stride + ch, acc);
}

// grad_bias[hk] = the sum of part[w][hk] over the workgroups w in ascending order: lane L adds its run of consecutive
// workgroups, lane 0 adds the 64 runs in lane order
__global__ __launch_bounds__(64) void k_lattn_bias_merge(const float *__restrict__ part, int64_t n_wg, int hk,
                                                        float *__restrict__ grad_bias) {
  __shared__ float s_run[64];
  const int64_t run = (n_wg + 63) / 64;
  const int64_t w0 = threadIdx.x * run, w1 = min(w0 + run, n_wg);
  float sum = 0.f;
  for (int64_t w = w0; w < w1; ++w) sum += part[w * hk + blockIdx.x];
  s_run[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.f;
    for (int t = 0; t < 64; ++t) total += s_run[t];
    grad_bias[blockIdx.x] = total;
  }
}

template <typename T, int D>
__global__ __launch_bounds__(kLattnThreads) void k_lattn_bwd_kv(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ dout,
    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t dout_stride, const int32_t *__restrict__ nbr_in,
    int64_t n_in, int volume, int heads, float scale, const float *__restrict__ bias, const float *__restrict__ lse,
    const float *__restrict__ lse_lo, const float *__restrict__ delta, T *__restrict__ dk, int64_t dk_stride, T *__restrict__ dv, int64_t dv_stride) {
  constexpr int V = 16 / (int)sizeof(T), G = D / V;
  int64_t item;
  int sub;
  const bool live = lattn_item<G>(n_in * heads, item, sub);
  const int64_t row = item / heads;
  const int head = (int)(item - row * heads);
  const int ch = head * D + sub * V;
  const Piece<V> kv = load_piece<T, V>(k + row * k_stride + ch);
  const Piece<V> vv = load_piece<T, V>(v + row * v_stride + ch);
  const float *bh = bias ? bias + (int64_t)head * volume : nullptr;
  const int32_t *col = nbr_in + row;
  int32_t i0 = col[0];
  int32_t i1 = col[(int64_t)min(1, volume - 1) * n_in];
  int64_t ic = max(i0, 0);
  Piece<V> qv = load_piece<T, V>(q + ic * q_stride + ch);
  Piece<V> gv = load_piece<T, V>(dout + ic * dout_stride + ch);
  float ls = lse[ic * heads + head], lo = lse_lo ? lse_lo[ic * heads + head] : 0.f, dl = delta[ic * heads + head];
  Piece<V> acc_k, acc_v;
#pragma unroll
  for (int j = 0; j < V; ++j) acc_k.v[j] = acc_v.v[j] = 0.f;
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t i2 = col[(int64_t)min(kk + 2, volume - 1) * n_in];
    ic = max(i1, 0);
    const Piece<V> qn = load_piece<T, V>(q + ic * q_stride + ch);
    const Piece<V> gn = load_piece<T, V>(dout + ic * dout_stride + ch);
    const float lsn = lse[ic * heads + head], lon = lse_lo ? lse_lo[ic * heads + head] : 0.f, dln = delta[ic * heads + head];
    const bool has = i0 >= 0;
    const float dot = lattn_dot<V, G>(qv, kv);
    const float dp = lattn_dot<V, G>(gv, vv);
    const float s = lattn_score(scale, dot, bh ? bh[kk] : 0.f);
    const float p = has ? expf((s - ls) - lo) : 0.f;
    const float ds = has ? p * (dp - dl) : 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      acc_v.v[j] = has ? fmaf(p, gv.v[j], acc_v.v[j]) : acc_v.v[j];
      acc_k.v[j] = has ? fmaf(ds, qv.v[j], acc_k.v[j]) : acc_k.v[j];
    }
    i0 = i1;
    i1 = i2;
    qv = qn;
    gv = gn;
    ls = lsn;
    lo = lon;
    dl = dln;
  }
  if (!live) return;
  if (dv != nullptr) store_piece<T, V>(dv + row * dv_stride + ch, acc_v);
  if (dk != nullptr) {
#pragma unroll
    for (int j = 0; j < V; ++j) acc_k.v[j] *= scale;
    store_piece<T, V>(dk + row * dk_stride + ch, acc_k);
  }
}

struct LattnArgs {
  const void *q, *k, *v, *out, *dout;
  int64_t q_stride, k_stride, v_stride, out_stride, dout_stride, dq_stride, dk_stride, dv_stride;
  const int32_t *nbr_out, *nbr_in;
  int64_t n_out, n_in;
  int volume, heads;
  float scale;
  const float *bias;
  float *lse, *lse_lo, *delta, *bias_part, *grad_bias;
  void *out_w, *dq, *dk, *dv;
};

// workgroups of a launch over `rows` target rows: a function of the shapes only
template <typename T, int D>
static int64_t lattn_grid(int64_t rows, int heads) {
  return ceil_div(rows * heads, kLattnThreads / (D / (16 / (int)sizeof(T))));
}

template <typename T, int D>
static int lattn_forward_t(const LattnArgs &a, hipStream_t stream) {
  k_lattn_fwd<T, D><<<(unsigned)lattn_grid<T, D>(a.n_out, a.heads), kLattnThreads, 0, stream>>>(
      (const T *)a.q, (const T *)a.k, (const T *)a.v, a.q_stride, a.k_stride, a.v_stride, a.nbr_out, a.n_out, a.volume,
      a.heads, a.scale, a.bias, (T *)a.out_w, a.out_stride, a.lse, a.lse_lo);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, int D>
static int lattn_backward_t(const LattnArgs &a, hipStream_t stream) {
  // delta is needed by both sides; the walk over the offsets is skipped inside when neither dq nor the bias wants it
  const int64_t n_wg = lattn_grid<T, D>(a.n_out, a.heads);
  k_lattn_bwd_q<T, D><<<(unsigned)n_wg, kLattnThreads, 0, stream>>>(
      (const T *)a.q, (const T *)a.k, (const T *)a.v, (const T *)a.out, (const T *)a.dout, a.q_stride, a.k_stride,
      a.v_stride, a.out_stride, a.dout_stride, a.nbr_out, a.n_out, a.volume, a.heads, a.scale, a.bias, a.lse, a.lse_lo,
      a.delta, (T *)a.dq, a.dq_stride, a.grad_bias ? a.bias_part : nullptr);
  ME_LAUNCH_CHECK();
  if (a.grad_bias) {
    k_lattn_bias_merge<<<(unsigned)(a.heads * a.volume), 64, 0, stream>>>(a.bias_part, n_wg, a.heads * a.volume,
                                                                         a.grad_bias);
    ME_LAUNCH_CHECK();
  }
  if ((a.dk || a.dv) && a.n_in > 0) {
    k_lattn_bwd_kv<T, D><<<(unsigned)lattn_grid<T, D>(a.n_in, a.heads), kLattnThreads, 0, stream>>>(
        (const T *)a.q, (const T *)a.k, (const T *)a.v, (const T *)a.dout, a.q_stride, a.k_stride, a.v_stride,
        a.dout_stride, a.nbr_in, a.n_in, a.volume, a.heads, a.scale, a.bias, a.lse, a.lse_lo, a.delta, (T *)a.dk, a.dk_stride,
        (T *)a.dv, a.dv_stride);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

#define ME_LATTN_DISPATCH_D(T, d, fn, ...)         \
  switch (d) {                                     \
    case 8: return fn<T, 8>(__VA_ARGS__);          \
    case 16: return fn<T, 16>(__VA_ARGS__);        \
    case 32: return fn<T, 32>(__VA_ARGS__);        \
    case 64: return fn<T, 64>(__VA_ARGS__);        \
    default: return fn<T, 128>(__VA_ARGS__);       \
  }
#define ME_LATTN_DISPATCH(is_bf16, d, fn, ...)                   \
  do {                                                           \
    if (is_bf16) { ME_LATTN_DISPATCH_D(__bf16, d, fn, __VA_ARGS__) } \
    ME_LATTN_DISPATCH_D(float, d, fn, __VA_ARGS__)               \
  } while (0)

// ---- float64 twins: plain double, one thread per (target row, head), the offsets in ascending k --------------------
__global__ __launch_bounds__(256) void k_lattn_fwd_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v, int64_t q_stride,
    int64_t k_stride, int64_t v_stride, const int32_t *__restrict__ nbr, int64_t n_out, int volume, int heads, int d,
    double scale, const double *__restrict__ bias, double *__restrict__ out, int64_t out_stride,
    double *__restrict__ lse) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_out * heads) return;
  const int64_t row = id / heads;
  const int head = (int)(id - row * heads);
  const double *qp = q + row * q_stride + (int64_t)head * d;
  double *op = out + row * out_stride + (int64_t)head * d;
  for (int c = 0; c < d; ++c) op[c] = 0.0;
  double m = -INFINITY;
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t j = nbr[(int64_t)kk * n_out + row];
    if (j < 0) continue;
    const double *kp = k + (int64_t)j * k_stride + (int64_t)head * d;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += qp[c] * kp[c];
    m = fmax(m, s * scale + (bias ? bias[(int64_t)head * volume + kk] : 0.0));
  }
  double l = 0.0;
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t j = nbr[(int64_t)kk * n_out + row];
    if (j < 0) continue;
    const double *kp = k + (int64_t)j * k_stride + (int64_t)head * d;
    const double *vp = v + (int64_t)j * v_stride + (int64_t)head * d;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += qp[c] * kp[c];
    const double p = exp(s * scale + (bias ? bias[(int64_t)head * volume + kk] : 0.0) - m);
    l += p;
    for (int c = 0; c < d; ++c) op[c] += p * vp[c];
  }
  if (l > 0.0)
    for (int c = 0; c < d; ++c) op[c] /= l;
  lse[id] = l > 0.0 ? m + log(l) : -INFINITY;
}

__global__ __launch_bounds__(256) void k_lattn_bwd_q_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v,
    const double *__restrict__ out, const double *__restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
    int64_t out_stride, int64_t dout_stride, const int32_t *__restrict__ nbr, int64_t n_out, int volume, int heads, int d,
    double scale, const double *__restrict__ bias, const double *__restrict__ lse, double *__restrict__ dq,
    int64_t dq_stride) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_out * heads) return;
  const int64_t row = id / heads;
  const int head = (int)(id - row * heads);
  const double *qp = q + row * q_stride + (int64_t)head * d;
  const double *op = out + row * out_stride + (int64_t)head * d;
  const double *gp = dout + row * dout_stride + (int64_t)head * d;
  double *dp = dq + row * dq_stride + (int64_t)head * d;
  const double ls = lse[id];
  double delta = 0.0;
  for (int c = 0; c < d; ++c) {
    delta += gp[c] * op[c];
    dp[c] = 0.0;
  }
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t j = nbr[(int64_t)kk * n_out + row];
    if (j < 0) continue;
    const double *kp = k + (int64_t)j * k_stride + (int64_t)head * d;
    const double *vp = v + (int64_t)j * v_stride + (int64_t)head * d;
    double s = 0.0, dpv = 0.0;
    for (int c = 0; c < d; ++c) {
      s += qp[c] * kp[c];
      dpv += gp[c] * vp[c];
    }
    const double p = exp(s * scale + (bias ? bias[(int64_t)head * volume + kk] : 0.0) - ls);
    const double ds = p * (dpv - delta) * scale;
    for (int c = 0; c < d; ++c) dp[c] += ds * kp[c];
  }
}

__global__ __launch_bounds__(256) void k_lattn_bwd_kv_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v,
    const double *__restrict__ out, const double *__restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
    int64_t out_stride, int64_t dout_stride, const int32_t *__restrict__ nbr_in, int64_t n_in, int volume, int heads,
    int d, double scale, const double *__restrict__ bias, const double *__restrict__ lse, double *__restrict__ dk,
    int64_t dk_stride, double *__restrict__ dv, int64_t dv_stride) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_in * heads) return;
  const int64_t row = id / heads;
  const int head = (int)(id - row * heads);
  const double *kp = k + row * k_stride + (int64_t)head * d;
  const double *vp = v + row * v_stride + (int64_t)head * d;
  double *dkp = dk ? dk + row * dk_stride + (int64_t)head * d : nullptr;
  double *dvp = dv ? dv + row * dv_stride + (int64_t)head * d : nullptr;
  for (int c = 0; c < d; ++c) {
    if (dkp) dkp[c] = 0.0;
    if (dvp) dvp[c] = 0.0;
  }
  for (int kk = 0; kk < volume; ++kk) {
    const int32_t i = nbr_in[(int64_t)kk * n_in + row];
    if (i < 0) continue;
    const double *qp = q + (int64_t)i * q_stride + (int64_t)head * d;
    const double *op = out + (int64_t)i * out_stride + (int64_t)head * d;
    const double *gp = dout + (int64_t)i * dout_stride + (int64_t)head * d;
    double s = 0.0, dpv = 0.0, delta = 0.0;
    for (int c = 0; c < d; ++c) {
      s += qp[c] * kp[c];
      dpv += gp[c] * vp[c];
      delta += gp[c] * op[c];
    }
    const double p = exp(s * scale + (bias ? bias[(int64_t)head * volume + kk] : 0.0) - lse[(int64_t)i * heads + head]);
    const double ds = p * (dpv - delta) * scale;
    for (int c = 0; c < d; ++c) {
      if (dvp) dvp[c] += p * gp[c];
      if (dkp) dkp[c] += ds * qp[c];
    }
  }
}

// grad_bias[h, k] = sum over the out rows i in ascending order of ds_ik: one thread per (h, k)
__global__ __launch_bounds__(64) void k_lattn_bwd_bias_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v,
    const double *__restrict__ out, const double *__restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
    int64_t out_stride, int64_t dout_stride, const int32_t *__restrict__ nbr, int64_t n_out, int volume, int heads, int d,
    double scale, const double *__restrict__ bias, const double *__restrict__ lse, double *__restrict__ grad_bias) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= heads * volume) return;
  const int head = id / volume, kk = id - head * volume;
  double sum = 0.0;
  for (int64_t row = 0; row < n_out; ++row) {
    const int32_t j = nbr[(int64_t)kk * n_out + row];
    if (j < 0) continue;
    const double *qp = q + row * q_stride + (int64_t)head * d;
    const double *op = out + row * out_stride + (int64_t)head * d;
    const double *gp = dout + row * dout_stride + (int64_t)head * d;
    const double *kp = k + (int64_t)j * k_stride + (int64_t)head * d;
    const double *vp = v + (int64_t)j * v_stride + (int64_t)head * d;
    double s = 0.0, dpv = 0.0, delta = 0.0;
    for (int c = 0; c < d; ++c) {
      s += qp[c] * kp[c];
      dpv += gp[c] * vp[c];
      delta += gp[c] * op[c];
    }
    sum += exp(s * scale + (bias ? bias[id] : 0.0) - lse[row * heads + head]) * (dpv - delta);
  }
  grad_bias[id] = sum;
}

static bool lattn_pow2_head(int d) { return d == 8 || d == 16 || d == 32 || d == 64 || d == 128; }

}  // namespace me

using namespace me;

// the argument checks shared by the entry points; `unit`: elements of 16 bytes (0: float64, any stride >= c)
#define ME_LATTN_CHECK_DIMS(unit)                                                                                      \
  ME_CHECK(n_out >= 0 && n_in >= 0 && n_out < (1ll << 31) && n_in < (1ll << 31), "bad row count");                     \
  ME_CHECK(heads > 0 && heads <= 65535 && c > 0, "bad head or channel count");                                         \
  ME_CHECK(c % heads == 0, "the channel count must be a multiple of the head count");                                  \
  ME_CHECK((unit) == 0 || lattn_pow2_head(c / heads),                                                                  \
           "the head dimension must be a power of two from 8 to 128 (any on the float64 entry points)");               \
  ME_CHECK(volume >= 1 && volume <= (1 << 20) && (int64_t)heads * volume < (1ll << 31), "kernel volume out of range"); \
  ME_CHECK((n_out + n_in) * (int64_t)heads < (1ll << 34), "too many (row, head) items")
#define ME_LATTN_CHECK_STRIDE(s, unit)                                                                                 \
  ME_CHECK((s) >= c && ((unit) == 0 || (s) % (unit) == 0), "a row stride must be >= the channel count and a multiple of 16 bytes")

extern "C" {

int64_t me_local_attn_workspace_bytes(int64_t n_out, int32_t heads, int64_t volume, int32_t with_bias) {
  const int64_t items = (n_out > 0 ? n_out : 0) * (int64_t)(heads > 0 ? heads : 0);
  int64_t bytes = align_up(items * (int64_t)sizeof(float), 256);   // delta [n_out, heads]
  if (with_bias)   // the sums of every workgroup of k_lattn_bwd_q [workgroups, heads, volume], at the fewest items a workgroup
    bytes += align_up(ceil_div(items, kLattnMinItems) * (int64_t)(heads > 0 ? heads : 0) * (volume > 0 ? volume : 0) *
                          (int64_t)sizeof(float), 256);
  return bytes;
}

int me_local_attn_forward(const void *q, const void *k, const void *v, int32_t is_bf16, int64_t q_stride,
                          int64_t k_stride, int64_t v_stride, const int32_t *nbr_out, int64_t n_out, int64_t n_in,
                          int64_t volume, int32_t c, int32_t heads, float scale, const float *rel_pos_bias, void *out,
                          int64_t out_stride, float *lse, float *lse_lo, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int unit = is_bf16 ? 8 : 4;
  ME_LATTN_CHECK_DIMS(unit);
  ME_LATTN_CHECK_STRIDE(q_stride, unit);
  ME_LATTN_CHECK_STRIDE(k_stride, unit);
  ME_LATTN_CHECK_STRIDE(v_stride, unit);
  ME_LATTN_CHECK_STRIDE(out_stride, unit);
  ME_CHECK(nbr_out != nullptr, "missing table pointer (the neighbour table of the out map)");
  if (n_out == 0) return 0;
  ME_CHECK(n_in > 0, "out rows need an in map with rows");
  ME_CHECK(q != nullptr && k != nullptr && v != nullptr && out != nullptr && lse != nullptr, "null data pointer");
  ME_CHECK(aligned({q, k, v, out}, 16), "q, k, v and out must be 16-byte aligned");
  LattnArgs a{};
  a.q = q; a.k = k; a.v = v;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride; a.out_stride = out_stride;
  a.nbr_out = nbr_out; a.n_out = n_out; a.n_in = n_in; a.volume = (int)volume; a.heads = heads; a.scale = scale;
  a.bias = rel_pos_bias; a.out_w = out; a.lse = lse; a.lse_lo = lse_lo;
  ME_LATTN_DISPATCH(is_bf16, c / heads, lattn_forward_t, a, stream);
}

int me_local_attn_backward(const void *q, const void *k, const void *v, const void *out, const float *lse,
                           const float *lse_lo, const void *dout, int32_t is_bf16, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                           int64_t out_stride, int64_t dout_stride, const int32_t *nbr_out, const int32_t *nbr_in,
                           int64_t n_out, int64_t n_in, int64_t volume, int32_t c, int32_t heads, float scale,
                           const float *rel_pos_bias, void *dq, int64_t dq_stride, void *dk, int64_t dk_stride, void *dv,
                           int64_t dv_stride, float *grad_rel_pos_bias, void *workspace, int64_t workspace_bytes,
                           void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int unit = is_bf16 ? 8 : 4;
  ME_LATTN_CHECK_DIMS(unit);
  ME_LATTN_CHECK_STRIDE(q_stride, unit);
  ME_LATTN_CHECK_STRIDE(k_stride, unit);
  ME_LATTN_CHECK_STRIDE(v_stride, unit);
  ME_LATTN_CHECK_STRIDE(out_stride, unit);
  ME_LATTN_CHECK_STRIDE(dout_stride, unit);
  ME_CHECK(dq == nullptr || (dq_stride >= c && dq_stride % unit == 0), "dq: a row stride must be >= the channel count and a multiple of 16 bytes");
  ME_CHECK(dk == nullptr || (dk_stride >= c && dk_stride % unit == 0), "dk: a row stride must be >= the channel count and a multiple of 16 bytes");
  ME_CHECK(dv == nullptr || (dv_stride >= c && dv_stride % unit == 0), "dv: a row stride must be >= the channel count and a multiple of 16 bytes");
  ME_CHECK(workspace_bytes >= me_local_attn_workspace_bytes(n_out, heads, volume, grad_rel_pos_bias != nullptr),
           "workspace too small");
  ME_CHECK(nbr_out != nullptr && nbr_in != nullptr, "missing table pointer (the neighbour tables of the out and in maps)");
  if (dq == nullptr && dk == nullptr && dv == nullptr && grad_rel_pos_bias == nullptr) return 0;
  if (n_out == 0) {   // keys without queries: zero gradients
    const size_t e = is_bf16 ? 2 : 4;
    if (dk && n_in > 0) ME_HIP(hipMemset2DAsync(dk, (size_t)dk_stride * e, 0, (size_t)c * e, (size_t)n_in, stream));
    if (dv && n_in > 0) ME_HIP(hipMemset2DAsync(dv, (size_t)dv_stride * e, 0, (size_t)c * e, (size_t)n_in, stream));
    if (grad_rel_pos_bias) ME_HIP(hipMemsetAsync(grad_rel_pos_bias, 0, (size_t)heads * volume * sizeof(float), stream));
    return 0;
  }
  ME_CHECK(n_in > 0, "out rows need an in map with rows");
  ME_CHECK(q != nullptr && k != nullptr && v != nullptr && out != nullptr && lse != nullptr && dout != nullptr &&
               workspace != nullptr,
           "null data pointer");
  ME_CHECK(aligned({q, k, v, out, dout, dq, dk, dv, workspace}, 16),
           "q, k, v, out, dout, the gradients and the workspace must be 16-byte aligned");
  LattnArgs a{};
  a.q = q; a.k = k; a.v = v; a.out = out; a.dout = dout;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride; a.out_stride = out_stride;
  a.dout_stride = dout_stride; a.dq_stride = dq_stride; a.dk_stride = dk_stride; a.dv_stride = dv_stride;
  a.nbr_out = nbr_out; a.nbr_in = nbr_in; a.n_out = n_out; a.n_in = n_in; a.volume = (int)volume; a.heads = heads;
  a.scale = scale; a.bias = rel_pos_bias;
  a.dq = dq; a.dk = dk; a.dv = dv; a.grad_bias = grad_rel_pos_bias;
  a.lse = const_cast<float *>(lse);
  a.lse_lo = const_cast<float *>(lse_lo);
  a.delta = reinterpret_cast<float *>(workspace);
  a.bias_part = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) +
                                          align_up(n_out * (int64_t)heads * (int64_t)sizeof(float), 256));
  ME_LATTN_DISPATCH(is_bf16, c / heads, lattn_backward_t, a, stream);
}

int me_local_attn_forward_f64(const double *q, const double *k, const double *v, int64_t q_stride, int64_t k_stride,
                              int64_t v_stride, const int32_t *nbr_out, int64_t n_out, int64_t n_in, int64_t volume,
                              int32_t c, int32_t heads, double scale, const double *rel_pos_bias, double *out,
                              int64_t out_stride, double *lse, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_LATTN_CHECK_DIMS(0);
  ME_LATTN_CHECK_STRIDE(q_stride, 0);
  ME_LATTN_CHECK_STRIDE(k_stride, 0);
  ME_LATTN_CHECK_STRIDE(v_stride, 0);
  ME_LATTN_CHECK_STRIDE(out_stride, 0);
  ME_CHECK(nbr_out != nullptr, "missing table pointer (the neighbour table of the out map)");
  if (n_out == 0) return 0;
  ME_CHECK(n_in > 0, "out rows need an in map with rows");
  ME_CHECK(q != nullptr && k != nullptr && v != nullptr && out != nullptr && lse != nullptr, "null data pointer");
  k_lattn_fwd_f64<<<(unsigned)ceil_div(n_out * heads, 256), 256, 0, stream>>>(
      q, k, v, q_stride, k_stride, v_stride, nbr_out, n_out, (int)volume, heads, c / heads, scale, rel_pos_bias, out,
      out_stride, lse);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_local_attn_backward_f64(const double *q, const double *k, const double *v, const double *out, const double *lse,
                               const double *dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int64_t out_stride, int64_t dout_stride, const int32_t *nbr_out, const int32_t *nbr_in,
                               int64_t n_out, int64_t n_in, int64_t volume, int32_t c, int32_t heads, double scale,
                               const double *rel_pos_bias, double *dq, int64_t dq_stride, double *dk, int64_t dk_stride,
                               double *dv, int64_t dv_stride, double *grad_rel_pos_bias, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_LATTN_CHECK_DIMS(0);
  ME_LATTN_CHECK_STRIDE(q_stride, 0);
  ME_LATTN_CHECK_STRIDE(k_stride, 0);
  ME_LATTN_CHECK_STRIDE(v_stride, 0);
  ME_LATTN_CHECK_STRIDE(out_stride, 0);
  ME_LATTN_CHECK_STRIDE(dout_stride, 0);
  ME_CHECK((dq == nullptr || dq_stride >= c) && (dk == nullptr || dk_stride >= c) && (dv == nullptr || dv_stride >= c),
           "a gradient row stride must be >= the channel count");
  ME_CHECK(nbr_out != nullptr && nbr_in != nullptr, "missing table pointer (the neighbour tables of the out and in maps)");
  if (n_out == 0) {
    if (dk && n_in > 0) ME_HIP(hipMemset2DAsync(dk, (size_t)dk_stride * 8, 0, (size_t)c * 8, (size_t)n_in, stream));
    if (dv && n_in > 0) ME_HIP(hipMemset2DAsync(dv, (size_t)dv_stride * 8, 0, (size_t)c * 8, (size_t)n_in, stream));
    if (grad_rel_pos_bias) ME_HIP(hipMemsetAsync(grad_rel_pos_bias, 0, (size_t)heads * volume * sizeof(double), stream));
    return 0;
  }
  ME_CHECK(n_in > 0, "out rows need an in map with rows");
  ME_CHECK(q != nullptr && k != nullptr && v != nullptr && out != nullptr && lse != nullptr && dout != nullptr,
           "null data pointer");
  if (dk || dv) {
    k_lattn_bwd_kv_f64<<<(unsigned)ceil_div(n_in * heads, 256), 256, 0, stream>>>(
        q, k, v, out, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, nbr_in, n_in, (int)volume, heads,
        c / heads, scale, rel_pos_bias, lse, dk, dk_stride, dv, dv_stride);
    ME_LAUNCH_CHECK();
  }
  if (dq) {
    k_lattn_bwd_q_f64<<<(unsigned)ceil_div(n_out * heads, 256), 256, 0, stream>>>(
        q, k, v, out, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, nbr_out, n_out, (int)volume, heads,
        c / heads, scale, rel_pos_bias, lse, dq, dq_stride);
    ME_LAUNCH_CHECK();
  }
  if (grad_rel_pos_bias) {
    k_lattn_bwd_bias_f64<<<(unsigned)ceil_div((int64_t)heads * volume, 64), 64, 0, stream>>>(
        q, k, v, out, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, nbr_out, n_out, (int)volume, heads,
        c / heads, scale, rel_pos_bias, lse, grad_rel_pos_bias);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
