// Instance normalisation over the rows of a sparse tensor's feature matrix [n, c] for gfx950 (MI355X).
//
// The reference's MinkowskiInstanceNorm (MinkowskiEngine/MinkowskiNormalization.py:194-399) is a chain of its global
// average pooling and broadcast operators plus torch element-wise ops: about 11 passes over the matrix forward and about
// 20 backward, each its own launch.  It is batch norm's arithmetic (norm.hip) with the statistics SEGMENTED by the batch
// index of each row (batch_row[i], the origin-map row of row i), so it gets batch norm's pipeline with that segmentation:
//
//   statistics  k_in_partial      one workgroup per chunk of consecutive rows.  Rows of an instance are normally
//                                 consecutive, so nearly every chunk holds ONE batch index: a thread owns a 16-byte channel
//                                 piece and strides over the rows (k_bn_partial's layout), shifted sums -> (count, mean, M2)
//                                 of (chunk, instance, channel).  A chunk that mixes batch indices runs the same loop once
//                                 per index present with the other rows masked (any row order is correct; the straddling
//                                 chunk of two consecutive instances reads its rows twice, from L2)
//               k_in_final        one wave per (instance, channel): the chunks that hold rows of the instance combined
//                                 with Chan's formula in a FIXED order -> mean, rstd = 1 / sqrt(biased variance + eps)
//   forward     k_seg_rows<InFwd> y = (x - mean[b]) * rstd[b] * gamma + beta; the coefficients of an instance stay in
//                                 registers while consecutive rows of the thread share the batch index (the row tile
//                                 seg_rows of segment_norm.hpp with the map InFwd)
//   backward    k_in_bwd_partial / k_in_bwd_final   t1[b] = sum dy, t2[b] = sum dy * xhat per (instance, channel)
//               k_in_bwd_params   grad_beta = sum_b t1[b], grad_gamma = sum_b t2[b] (ascending b)
//               k_seg_rows<InBwd> dx = gamma * rstd[b] * (dy - t1[b] / n_b - xhat * t2[b] / n_b)
// No atomics on values, every sum in a fixed order: bitwise reproducible.  T = float or __bf16 rows; statistics and
// parameters fp32.  The float64 twins at the end are the gradcheck yardstick (plain double, one thread per output).
#include "segment_norm.hpp"

namespace me {

// The scans of a chunk, the bodies of the two-level reductions, the row tile and the workspace are segment_norm.hpp's
// (shared with group_norm.hip); the kernels and maps here are theirs for one record per (instance, channel).
template <typename T, int V>
__global__ __launch_bounds__(256) void k_in_partial(const T *__restrict__ x, const int32_t *__restrict__ batch_row,
                                                   int64_t n, int c, int chunks, int n_batch,
                                                   float *__restrict__ part_mean, float *__restrict__ part_m2,
                                                   float *__restrict__ part_cnt) {
  extern __shared__ float s_red[];  // in_partial_lds_bytes
  seg_partial<T, V>(s_red, x, batch_row, n, c, chunks, n_batch, part_mean, part_m2, part_cnt);
}

// One wave per (instance b, channel): seg_merge_chunks -> mean, rstd = 1 / sqrt(biased variance + eps).
// An instance without rows on this map: mean = 0, rstd = 1 / sqrt(eps).
__global__ __launch_bounds__(256) void k_in_final(const float *__restrict__ part_mean, const float *__restrict__ part_m2,
                                                 const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                 float eps, float *__restrict__ mean_out, float *__restrict__ rstd_out) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b, channel)
  if (idx >= (int64_t)n_batch * c) return;  // whole wave
  SegMerge m;
  if (!seg_merge_chunks(part_mean, part_m2, part_cnt, chunks, n_batch, c, (int)(idx / c), (int)(idx % c), m)) {
    if (lane == 0) {
      mean_out[idx] = 0.f;
      rstd_out[idx] = 1.f / sqrtf(eps);
    }
    return;
  }
  if (lane != 0) return;
  const float am = m.sa / m.sn;
  const float var = clamp_neg(m.sb - m.sa * am) / m.sn;
  mean_out[idx] = m.shift + am;
  rstd_out[idx] = 1.f / sqrtf(var + eps);
}

// y = (x - mean[b]) * (rstd[b] * gamma) + beta (gamma / beta may be NULL: 1 / 0): the forward map of seg_rows.
// mean / rstd: [n_batch][c]
struct InFwd {
  static constexpr bool kDy = false;
  const float *mean, *rstd, *gamma, *beta;
  int c;
  template <int V>
  struct Piece {
    float ga[V], be[V], a[V], mu[V];
  };
  template <int V>
  __device__ __forceinline__ void init(int ch0, Piece<V> &pc) const {
    load_affine<V>(gamma, beta, ch0, pc.ga, pc.be);
  }
  template <int V>
  __device__ __forceinline__ void load(int b, int ch0, Piece<V> &pc) const {
    load_f32<V>(mean + (int64_t)b * c + ch0, pc.mu);
    load_f32<V>(rstd + (int64_t)b * c + ch0, pc.a);
#pragma unroll
    for (int j = 0; j < V; ++j) pc.a[j] *= pc.ga[j];
  }
  template <int V>
  __device__ __forceinline__ float value(const Piece<V> &pc, int j, float x) const {
    return fmaf(x - pc.mu[j], pc.a[j], pc.be[j]);
  }
};

// mean / rstd of instance b for V channels from ch0: [n_batch][c]
struct InCoef {
  const float *mean, *rstd;
  int c;
  template <int V>
  __device__ __forceinline__ void operator()(int b, int ch0, float (&m)[V], float (&rs)[V]) const {
    load_f32<V>(mean + (int64_t)b * c + ch0, m);
    load_f32<V>(rstd + (int64_t)b * c + ch0, rs);
  }
};

// per (chunk, instance, channel): sum dy and sum dy * xhat (xhat = (x - mean[b]) * rstd[b]); layout of k_in_partial
template <typename T, int V>
__global__ __launch_bounds__(256) void k_in_bwd_partial(const T *__restrict__ x, const T *__restrict__ dy,
                                                       const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                       int chunks, int n_batch, const float *__restrict__ mean,
                                                       const float *__restrict__ rstd, float *__restrict__ part_dy,
                                                       float *__restrict__ part_dyx, float *__restrict__ part_cnt) {
  extern __shared__ float s_red[];  // in_partial_lds_bytes
  seg_bwd_partial<T, V>(s_red, x, dy, batch_row, n, c, chunks, n_batch, InCoef{mean, rstd, c}, part_dy, part_dyx,
                        part_cnt);
}

// t1 = sum dy, t2 = sum dy * xhat per (instance, channel) and rows[b]: one wave each over the chunks, a fixed order
__global__ __launch_bounds__(256) void k_in_bwd_final(const float *__restrict__ part_dy,
                                                     const float *__restrict__ part_dyx,
                                                     const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                     float *__restrict__ t1, float *__restrict__ t2,
                                                     float *__restrict__ rows) {
  seg_bwd_final(part_dy, part_dyx, part_cnt, chunks, n_batch, c, t1, t2, rows);
}

// grad_beta = sum over the instances (ascending) of t1, grad_gamma = of t2; either may be NULL
__global__ __launch_bounds__(256) void k_in_bwd_params(const float *__restrict__ t1, const float *__restrict__ t2,
                                                      int n_batch, int c, float *__restrict__ grad_gamma,
                                                      float *__restrict__ grad_beta) {
  seg_bwd_params<float>(t1, t2, n_batch, c, grad_gamma, grad_beta);
}

// dx = A * ((dy - k1) - (x - mean[b]) * k2) with A = gamma * rstd[b], k1 = t1[b] / n_b, k2 = t2[b] / n_b * rstd[b]: the
// backward map of seg_rows
struct InBwd {
  static constexpr bool kDy = true;
  const float *mean, *rstd, *gamma, *t1, *t2, *rows;
  int c;
  template <int V>
  struct Piece {
    float ga[V], A[V], k1[V], k2[V], mu[V];
  };
  template <int V>
  __device__ __forceinline__ void init(int ch0, Piece<V> &pc) const {
    float unused[V];
    load_affine<V>(gamma, nullptr, ch0, pc.ga, unused);
  }
  template <int V>
  __device__ __forceinline__ void load(int b, int ch0, Piece<V> &pc) const {
    const int64_t o = (int64_t)b * c + ch0;
    const float inv_n = 1.f / fmaxf(rows[b], 1.f);
    load_f32<V>(mean + o, pc.mu);
    load_f32<V>(rstd + o, pc.A);
    load_f32<V>(t1 + o, pc.k1);
    load_f32<V>(t2 + o, pc.k2);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      pc.k1[j] *= inv_n;
      pc.k2[j] *= inv_n * pc.A[j];
      pc.A[j] *= pc.ga[j];
    }
  }
  template <int V>
  __device__ __forceinline__ float value(const Piece<V> &pc, int j, float x, float dy) const {
    return pc.A[j] * ((dy - pc.k1[j]) - (x - pc.mu[j]) * pc.k2[j]);
  }
};

// ---- float64: the same formulae in plain double, one thread per output (gradcheck yardstick, not a hot path) ----------
// per (instance, channel): mean, then M2 about it, rows in ascending order
__global__ __launch_bounds__(256) void k_in_stats_f64(const double *__restrict__ x,
                                                     const int32_t *__restrict__ batch_row, int64_t n, int n_batch,
                                                     int c, double eps, double *__restrict__ mean,
                                                     double *__restrict__ rstd) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_batch * c) return;
  const int b = (int)(idx / c), ch = (int)(idx % c);
  double s = 0.0, cnt = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    if (batch_row[r] != b) continue;
    s += x[r * c + ch];
    cnt += 1.0;
  }
  const double m = cnt > 0.0 ? s / cnt : 0.0;
  double q = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    if (batch_row[r] != b) continue;
    const double d = x[r * c + ch] - m;
    q = fma(d, d, q);
  }
  mean[idx] = m;
  rstd[idx] = 1.0 / sqrt((cnt > 0.0 ? q / cnt : 0.0) + eps);
}

__global__ __launch_bounds__(256) void k_in_apply_f64(const double *__restrict__ x,
                                                     const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                     int n_batch, const double *__restrict__ mean,
                                                     const double *__restrict__ rstd, const double *__restrict__ gamma,
                                                     const double *__restrict__ beta, double *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * c) return;
  const int ch = (int)(idx % c);
  const int64_t o = (int64_t)min(max(batch_row[idx / c], 0), n_batch - 1) * c + ch;
  const double v = (x[idx] - mean[o]) * rstd[o];
  y[idx] = fma(v, gamma ? gamma[ch] : 1.0, beta ? beta[ch] : 0.0);
}

// t1[b] = sum dy, t2[b] = sum dy * xhat, rows[b]
__global__ __launch_bounds__(256) void k_in_bwd_sums_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                        const int32_t *__restrict__ batch_row, int64_t n, int n_batch,
                                                        int c, const double *__restrict__ mean,
                                                        const double *__restrict__ rstd, double *__restrict__ t1,
                                                        double *__restrict__ t2, double *__restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_batch * c) return;
  const int b = (int)(idx / c), ch = (int)(idx % c);
  const double m = mean[idx], rs = rstd[idx];
  double a = 0.0, q = 0.0, cnt = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    if (batch_row[r] != b) continue;
    const double g = dy[r * c + ch];
    a += g;
    q = fma(g, (x[r * c + ch] - m) * rs, q);
    cnt += 1.0;
  }
  t1[idx] = a;
  t2[idx] = q;
  if (ch == 0) rows[b] = cnt;
}

__global__ __launch_bounds__(256) void k_in_bwd_params_f64(const double *__restrict__ t1, const double *__restrict__ t2,
                                                          int n_batch, int c, double *__restrict__ grad_gamma,
                                                          double *__restrict__ grad_beta) {
  seg_bwd_params<double>(t1, t2, n_batch, c, grad_gamma, grad_beta);
}

__global__ __launch_bounds__(256) void k_in_bwd_apply_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                         const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                         int n_batch, const double *__restrict__ mean,
                                                         const double *__restrict__ rstd,
                                                         const double *__restrict__ gamma, const double *__restrict__ t1,
                                                         const double *__restrict__ t2, const double *__restrict__ rows,
                                                         double *__restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * c) return;
  const int ch = (int)(idx % c);
  const int b = min(max(batch_row[idx / c], 0), n_batch - 1);
  const int64_t o = (int64_t)b * c + ch;
  const double inv_n = 1.0 / fmax(rows[b], 1.0);
  const double xh = (x[idx] - mean[o]) * rstd[o];
  dx[idx] = (gamma ? gamma[ch] : 1.0) * rstd[o] * (dy[idx] - t1[o] * inv_n - xh * t2[o] * inv_n);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// workspace: in_ws_layout_f32 (the float64 entry points use t1 | t2 | rows as doubles at the start)
static int64_t in_ws_layout(int64_t n, int n_batch, int c, char *base, InWs *w) {
  const int64_t f32 = in_ws_layout_f32(n, n_batch, c, base, w);
  const int64_t f64 = 2 * align_up((int64_t)n_batch * c * 8, 256) + align_up((int64_t)n_batch * 8, 256);
  return f32 > f64 ? f32 : f64;
}

template <typename T>
static int in_stats(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, float eps, float *mean,
                    float *rstd, const InWs &w, hipStream_t stream) {
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread, {x});
  ME_CHECK(pl.lds <= 64 * 1024, "channel count too large for the instance-norm kernels");
  ME_HIP(hipMemsetAsync(w.cnt, 0, (size_t)pl.chunks * n_batch * 4, stream));
  if (n > 0)
    ME_PIECE_DISPATCH(T, kPieceNorm, pl.v,
                      hipLaunchKernelGGL((k_in_partial<T, V>), dim3(pl.chunks), dim3(256), pl.lds, stream, x, batch_row, n,
                                         c, pl.chunks, n_batch, w.pa, w.pb, w.cnt));
  hipLaunchKernelGGL(k_in_final, dim3((unsigned)ceil_div((int64_t)n_batch * c, 4)), dim3(256), 0, stream, w.pa, w.pb,
                     w.cnt, pl.chunks, n_batch, c, eps, mean, rstd);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int in_apply(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, const float *mean,
                    const float *rstd, const float *gamma, const float *beta, T *y, hipStream_t stream) {
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread, {x, y, mean, rstd});
  const InFwd map{mean, rstd, gamma, beta, c};
  ME_SEG_ROWS(T, pl, stream, x, (const T *)nullptr, batch_row, n, c, n_batch, map, y);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int in_backward(const T *x, const T *dy, const int32_t *batch_row, int64_t n, int n_batch, int c,
                       const float *mean, const float *rstd, const float *gamma, T *dx, float *grad_gamma,
                       float *grad_beta, const InWs &w, hipStream_t stream) {
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread / 2, {x, dy, dx, mean, rstd});
  ME_CHECK(pl.lds <= 64 * 1024, "channel count too large for the instance-norm kernels");
  ME_HIP(hipMemsetAsync(w.cnt, 0, (size_t)pl.chunks * n_batch * 4, stream));
  ME_PIECE_DISPATCH(T, kPieceNorm, pl.v,
                    hipLaunchKernelGGL((k_in_bwd_partial<T, V>), dim3(pl.chunks), dim3(256), pl.lds, stream, x, dy,
                                       batch_row, n, c, pl.chunks, n_batch, mean, rstd, w.pa, w.pb, w.cnt));
  hipLaunchKernelGGL(k_in_bwd_final, dim3((unsigned)ceil_div((int64_t)n_batch * c, 4)), dim3(256), 0, stream, w.pa, w.pb,
                     w.cnt, pl.chunks, n_batch, c, w.t1, w.t2, w.rows);
  if (grad_gamma != nullptr || grad_beta != nullptr)
    hipLaunchKernelGGL(k_in_bwd_params, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, stream, w.t1, w.t2, n_batch, c,
                       grad_gamma, grad_beta);
  if (dx != nullptr) {
    const InBwd map{mean, rstd, gamma, w.t1, w.t2, w.rows, c};
    ME_SEG_ROWS(T, pl, stream, x, dy, batch_row, n, c, n_batch, map, dx);
  }
  ME_LAUNCH_CHECK();
  return 0;
}

}  // namespace me

using namespace me;

#define ME_IN_CHECK_ARGS()                                                                                       \
  ME_CHECK(n >= 0 && c > 0 && n_batch > 0, "instance norm needs a channel count and at least one instance");     \
  ME_CHECK(n < (1ll << 40) && (int64_t)n_batch * c < (1ll << 31), "instance norm: matrix or statistics too large")

extern "C" {

int64_t me_inorm_workspace_bytes(int64_t n, int32_t n_batch, int32_t c) {
  return in_ws_layout(n < 0 ? 0 : n, n_batch, c, nullptr, nullptr);
}

int me_inorm_stats(const void *x, int32_t is_bf16, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                   float eps, float *mean, float *rstd, void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_IN_CHECK_ARGS();
  ME_CHECK(workspace_bytes >= me_inorm_workspace_bytes(n, n_batch, c), "workspace too small");
  InWs w;
  in_ws_layout(n, n_batch, c, reinterpret_cast<char *>(workspace), &w);
  ME_SEG_RETURN_T(is_bf16, in_stats<T>((const T *)x, batch_row, n, n_batch, c, eps, mean, rstd, w, stream));
}

int me_inorm_apply(const void *x, int32_t is_bf16, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                   const float *mean, const float *rstd, const float *gamma, const float *beta, void *y,
                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_IN_CHECK_ARGS();
  if (n == 0) return 0;
  ME_SEG_RETURN_T(is_bf16, in_apply<T>((const T *)x, batch_row, n, n_batch, c, mean, rstd, gamma, beta, (T *)y, stream));
}

int me_inorm_backward(const void *x, const void *dy, int32_t is_bf16, const int32_t *batch_row, int64_t n,
                      int32_t n_batch, int32_t c, const float *mean, const float *rstd, const float *gamma, void *dx,
                      float *grad_gamma, float *grad_beta, void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_IN_CHECK_ARGS();
  ME_CHECK(n > 0, "instance norm backward needs at least one row");
  ME_CHECK(workspace_bytes >= me_inorm_workspace_bytes(n, n_batch, c), "workspace too small");
  InWs w;
  in_ws_layout(n, n_batch, c, reinterpret_cast<char *>(workspace), &w);
  ME_SEG_RETURN_T(is_bf16, in_backward<T>((const T *)x, (const T *)dy, batch_row, n, n_batch, c, mean, rstd, gamma,
                                          (T *)dx, grad_gamma, grad_beta, w, stream));
}

int me_inorm_stats_f64(const double *x, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c, double eps,
                       double *mean, double *rstd, void *stream_) {
  ME_IN_CHECK_ARGS();
  hipLaunchKernelGGL(k_in_stats_f64, dim3((unsigned)ceil_div((int64_t)n_batch * c, 256)), dim3(256), 0,
                     (hipStream_t)stream_, x, batch_row, n, n_batch, c, eps, mean, rstd);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_inorm_apply_f64(const double *x, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                       const double *mean, const double *rstd, const double *gamma, const double *beta, double *y,
                       void *stream_) {
  ME_IN_CHECK_ARGS();
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_in_apply_f64, dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, (hipStream_t)stream_, x,
                     batch_row, n, c, n_batch, mean, rstd, gamma, beta, y);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_inorm_backward_f64(const double *x, const double *dy, const int32_t *batch_row, int64_t n, int32_t n_batch,
                          int32_t c, const double *mean, const double *rstd, const double *gamma, double *dx,
                          double *grad_gamma, double *grad_beta, void *workspace, int64_t workspace_bytes,
                          void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_IN_CHECK_ARGS();
  ME_CHECK(workspace_bytes >= me_inorm_workspace_bytes(n, n_batch, c), "workspace too small");
  const int64_t t = align_up((int64_t)n_batch * c * 8, 256);
  double *t1 = reinterpret_cast<double *>(workspace);
  double *t2 = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + t);
  double *rows = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + 2 * t);
  hipLaunchKernelGGL(k_in_bwd_sums_f64, dim3((unsigned)ceil_div((int64_t)n_batch * c, 256)), dim3(256), 0, stream, x, dy,
                     batch_row, n, n_batch, c, mean, rstd, t1, t2, rows);
  if (grad_gamma != nullptr || grad_beta != nullptr)
    hipLaunchKernelGGL(k_in_bwd_params_f64, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, stream, t1, t2, n_batch, c,
                       grad_gamma, grad_beta);
  if (dx != nullptr && n > 0)
    hipLaunchKernelGGL(k_in_bwd_apply_f64, dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, stream, x, dy, batch_row, n,
                       c, n_batch, mean, rstd, gamma, t1, t2, rows, dx);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_instance_norm(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::k_in_final));
}
