// Group normalisation over the rows of a sparse tensor's feature matrix [n, c] for gfx950 (MI355X): every instance
// (batch index) b and every group g of cg = c / groups consecutive channels is normalised with the mean and the biased
// variance of its n_b * cg values.  torch.nn.GroupNorm needs one dense tensor per sample; the rows of a sparse tensor are
// segmented by batch_row[i] with segments of different lengths, which is the segmentation instance_norm.hip solves
// (segment_norm.hpp), plus a merge over the channels of a group:
//
//   statistics  k_gn_partial      seg_partial: count / mean / M2 of (chunk, instance, channel) from shifted sums — the
//                                 row pass does not know about groups
//               k_gn_chan_final   one wave per (instance, channel): the chunks merged with Chan's formula relative to one
//                                 shift, in a fixed order -> the channel record (rows, mean_c, M2_c)
//               k_gn_group_final  one thread per (instance, group): the cg channel records in ascending channel order.
//                                 Their counts are equal, so mean_g is the mean of the mean_c (taken relative to the first
//                                 one) and M2_g = sum M2_c + n_b * sum (mean_c - mean_g)^2 -> mean, rstd [n_batch, groups]
//   forward     k_seg_rows<GnFwd> y = (x - mean[b, g]) * rstd[b, g] * gamma + beta: the row tile seg_rows of
//                                 segment_norm.hpp with the map GnFwd.  A thread owns a 16-byte channel piece, which may
//                                 straddle groups (cg = 3 with 4 floats, cg = 6 with 8 bf16): the group of every element
//                                 of the piece is computed once, outside the row loop; the coefficients of an instance
//                                 are re-read only when the batch index changes between two rows of the thread
//   backward    k_gn_bwd_partial / k_gn_bwd_final   t1[b, c] = sum dy, t2[b, c] = sum dy * xhat (seg_bwd_partial with the
//                                 group's mean / rstd)
//               k_gnc_bwd_params  grad_beta = sum_b t1, grad_gamma = sum_b t2 (ascending b): the conditional norm's kernel
//                                 without modulation
//               k_gn_bwd_group    T1[b, g] = sum_{c in g} gamma[c] * t1[b, c], T2 likewise (ascending c)
//               k_seg_rows<GnBwd> dx = rstd * (gamma * dy - T1 / m - xhat * T2 / m), m = n_b * cg
// The maps are templated on the source of the affine map (GnPerChannel: gamma / beta here; GnPerInstance: the conditional
// norm below) and on the activation; both norms share every kernel but k_gnc_coef.
// x is read twice and y written once forward; x and dy are read twice and dx written once backward, as instance norm.
// No atomics on values, every sum in a fixed order: bitwise reproducible.  T = float or __bf16 rows; statistics and
// parameters fp32.  The float64 twins at the end are the gradcheck yardstick (plain double, one thread per output).
#include "segment_norm.hpp"

namespace me {

template <typename T, int V>
__global__ __launch_bounds__(256) void k_gn_partial(const T *__restrict__ x, const int32_t *__restrict__ batch_row,
                                                   int64_t n, int c, int chunks, int n_batch,
                                                   float *__restrict__ part_mean, float *__restrict__ part_m2,
                                                   float *__restrict__ part_cnt) {
  extern __shared__ float s_red[];  // in_partial_lds_bytes
  seg_partial<T, V>(s_red, x, batch_row, n, c, chunks, n_batch, part_mean, part_m2, part_cnt);
}

// One wave per (instance b, channel): the channel record cmean / cm2 [n_batch][c] and rows[b] (0 / 0 / 0 for an instance
// without rows on this map, so that k_gn_group_final reads only words written here)
__global__ __launch_bounds__(256) void k_gn_chan_final(const float *__restrict__ part_mean,
                                                      const float *__restrict__ part_m2,
                                                      const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                      float *__restrict__ cmean, float *__restrict__ cm2,
                                                      float *__restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b, channel)
  if (idx >= (int64_t)n_batch * c) return;  // whole wave
  const int b = (int)(idx / c), ch = (int)(idx % c);
  SegMerge m;
  const bool have = seg_merge_chunks(part_mean, part_m2, part_cnt, chunks, n_batch, c, b, ch, m);   // uniform
  if (lane != 0) return;
  float mean = 0.f, m2 = 0.f, cnt = 0.f;
  if (have) {
    const float am = m.sa / m.sn;
    mean = m.shift + am;
    m2 = clamp_neg(m.sb - m.sa * am);
    cnt = m.sn;
  }
  cmean[idx] = mean;
  cm2[idx] = m2;
  if (ch == 0) rows[b] = cnt;
}

// One thread per (instance b, group g): the cg channel records of the group, ascending.  An instance without rows:
// mean = 0, rstd = 1 / sqrt(eps).
__global__ __launch_bounds__(256) void k_gn_group_final(const float *__restrict__ cmean, const float *__restrict__ cm2,
                                                       const float *__restrict__ rows, int n_batch, int c, int groups,
                                                       float eps, float *__restrict__ mean_out,
                                                       float *__restrict__ rstd_out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // (b, g)
  if (idx >= n_batch * groups) return;
  const int b = idx / groups, g = idx % groups, cg = c / groups;
  const float nb = rows[b];
  if (!(nb > 0.f)) {
    mean_out[idx] = 0.f;
    rstd_out[idx] = 1.f / sqrtf(eps);
    return;
  }
  const float *pm = cmean + (int64_t)b * c + g * cg, *pq = cm2 + (int64_t)b * c + g * cg;
  const float m0 = pm[0];
  float s = 0.f;
  for (int k = 0; k < cg; ++k) s += pm[k] - m0;
  const float mg = m0 + s / (float)cg;
  float q1 = 0.f, q2 = 0.f;
  for (int k = 0; k < cg; ++k) {
    const float d = pm[k] - mg;
    q1 += pq[k];
    q2 = fmaf(d, d, q2);
  }
  const float var = clamp_neg(fmaf(nb, q2, q1)) / (nb * (float)cg);
  mean_out[idx] = mg;
  rstd_out[idx] = 1.f / sqrtf(var + eps);
}

// the group of each of the V channels from ch0: fixed for a thread's piece, computed outside its row loop
template <int V>
__device__ __forceinline__ void gn_piece_groups(int ch0, int cg, int (&grp)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) grp[j] = (ch0 + j) / cg;
}

// mean / rstd [n_batch][groups] of instance b for the V channels from ch0
struct GnCoef {
  const float *mean, *rstd;
  int groups, cg;
  template <int V>
  __device__ __forceinline__ void operator()(int b, int ch0, float (&m)[V], float (&rs)[V]) const {
    int grp[V];
    gn_piece_groups<V>(ch0, cg, grp);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      m[j] = mean[b * groups + grp[j]];
      rs[j] = rstd[b * groups + grp[j]];
    }
  }
};

// per (chunk, instance, channel): sum g and sum g * xhat with xhat = (x - mean[b, g]) * rstd[b, g] and g the gradient
// that Grad makes of dy: SegGradPlain (dy itself) for the plain and the conditional norm without activation, GncGrad with
// the SiLU
template <typename T, int V, typename Grad>
__global__ __launch_bounds__(256) void k_gn_bwd_partial(const T *__restrict__ x, const T *__restrict__ dy,
                                                       const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                       int chunks, int n_batch, const GnCoef coef, const Grad grad,
                                                       float *__restrict__ part_dy, float *__restrict__ part_dyx,
                                                       float *__restrict__ part_cnt) {
  extern __shared__ float s_red[];  // in_partial_lds_bytes
  seg_bwd_partial<T, V>(s_red, x, dy, batch_row, n, c, chunks, n_batch, coef, part_dy, part_dyx, part_cnt, grad);
}

// t1 = sum dy, t2 = sum dy * xhat per (instance, channel) and rows[b]: one wave each over the chunks, a fixed order
__global__ __launch_bounds__(256) void k_gn_bwd_final(const float *__restrict__ part_dy,
                                                     const float *__restrict__ part_dyx,
                                                     const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                     float *__restrict__ t1, float *__restrict__ t2,
                                                     float *__restrict__ rows) {
  seg_bwd_final(part_dy, part_dyx, part_cnt, chunks, n_batch, c, t1, t2, rows);
}

// One thread per (instance b, group g): T1 = sum_{c in g} w[b, c] * t1[b, c], T2 = the same of t2, ascending c.  The
// weight of (b, c) is w[b * w_stride + c]: w_stride = 0 for gamma[c], c for ge[b, c]; w may be NULL: 1
template <typename F>
__global__ __launch_bounds__(256) void k_gn_bwd_group(const F *__restrict__ t1, const F *__restrict__ t2,
                                                     const F *__restrict__ w, int w_stride, int n_batch, int c,
                                                     int groups, F *__restrict__ g1, F *__restrict__ g2) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // (b, g)
  if (idx >= n_batch * groups) return;
  const int b = idx / groups, g = idx % groups, cg = c / groups;
  F a = 0, q = 0;
  for (int k = 0; k < cg; ++k) {
    const int ch = g * cg + k;
    const F wt = w != nullptr ? w[(int64_t)b * w_stride + ch] : (F)1;
    a = fma(wt, t1[(int64_t)b * c + ch], a);
    q = fma(wt, t2[(int64_t)b * c + ch], q);
  }
  g1[idx] = a;
  g2[idx] = q;
}

// a * b rounded on its own, never contracted into an fma with a neighbouring add
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---- float64: the same formulae in plain double, one thread per output (gradcheck yardstick, not a hot path) ----------
// per (instance, group): mean, then M2 about it, rows ascending and the channels of the group ascending within a row
__global__ __launch_bounds__(256) void k_gn_stats_f64(const double *__restrict__ x,
                                                     const int32_t *__restrict__ batch_row, int64_t n, int n_batch,
                                                     int c, int groups, double eps, double *__restrict__ mean,
                                                     double *__restrict__ rstd) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_batch * groups) return;
  const int b = idx / groups, g = idx % groups, cg = c / groups;
  double s = 0.0, cnt = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    if (batch_row[r] != b) continue;
    for (int k = 0; k < cg; ++k) s += x[r * c + g * cg + k];
    cnt += (double)cg;
  }
  const double m = cnt > 0.0 ? s / cnt : 0.0;
  double q = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    if (batch_row[r] != b) continue;
    for (int k = 0; k < cg; ++k) {
      const double d = x[r * c + g * cg + k] - m;
      q = fma(d, d, q);
    }
  }
  mean[idx] = m;
  rstd[idx] = 1.0 / sqrt((cnt > 0.0 ? q / cnt : 0.0) + eps);
}

// t1[b, c] = sum dy, t2[b, c] = sum dy * xhat, rows[b]
__global__ __launch_bounds__(256) void k_gn_bwd_sums_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                        const int32_t *__restrict__ batch_row, int64_t n, int n_batch,
                                                        int c, int groups, const double *__restrict__ mean,
                                                        const double *__restrict__ rstd, double *__restrict__ t1,
                                                        double *__restrict__ t2, double *__restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_batch * c) return;
  const int b = (int)(idx / c), ch = (int)(idx % c);
  const double m = mean[b * groups + ch / (c / groups)], rs = rstd[b * groups + ch / (c / groups)];
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

__global__ __launch_bounds__(256) void k_gn_bwd_apply_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                         const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                         int n_batch, int groups, const double *__restrict__ mean,
                                                         const double *__restrict__ rstd,
                                                         const double *__restrict__ gamma, const double *__restrict__ g1,
                                                         const double *__restrict__ g2, const double *__restrict__ rows,
                                                         double *__restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * c) return;
  const int ch = (int)(idx % c);
  const int b = min(max(batch_row[idx / c], 0), n_batch - 1);
  const int o = b * groups + ch / (c / groups);
  const double inv_m = 1.0 / fmax(rows[b] * (double)(c / groups), 1.0);
  const double xh = (x[idx] - mean[o]) * rstd[o];
  dx[idx] = rstd[o] * ((gamma ? gamma[ch] : 1.0) * dy[idx] - g1[o] * inv_m - xh * g2[o] * inv_m);
}

// ---- conditional group norm (MinkowskiConditionalGroupNorm): per-instance scale / shift and a fused SiLU -------------
//   v = xhat * ge[b, c] + be[b, c], ge = gamma * (1 + scale[b]), be = beta * (1 + scale[b]) + shift[b], y = act(v)
// The statistics are k_gn_partial / k_gn_chan_final / k_gn_group_final, unchanged.  The modulation is an affine map per
// (instance, channel): k_gnc_coef writes ge / be [n_batch][c] into the workspace once per call and every later kernel
// reads them where the plain norm reads gamma / beta — at a change of the batch index in the row maps, once per
// (instance, piece) in the partial kernel — so the row loops gain two coefficient loads and no arithmetic on
// gamma / beta / scale / shift.  With scale = shift = NULL and the identity, ge = gamma and be = beta bit for bit and
// every expression is the plain norm's.
//   k_gnc_coef                           one thread per (instance, channel)
//   k_seg_rows<GnFwd<GnPerInstance, ACT>>  SiLU in fp32, one rounding at a bf16 store
//   k_gn_bwd_partial<GncGrad>            with the SiLU: dv = dy * act'(v) in place of dy, v recomputed from x
//   k_gnc_bwd_params                     one thread per channel, ascending b: grad_shift = t1, grad_scale = gamma * t2 +
//                                        beta * t1, grad_beta = sum_b (1 + scale) * t1, grad_gamma = sum_b (1 + scale) * t2
//   k_gn_bwd_group                       with ge[b, c] in place of gamma[c]
//   k_seg_rows<GnBwd<GnPerInstance, ACT>>  with ge and dv
// Pass counts of group norm: x twice and y once forward; x and dy twice and dx once backward.  No atomics on values.
enum { kGncIdentity = 0, kGncSilu = 1 };

// SiLU and its derivative from one sigmoid: s = 1 / (1 + exp(-v)); exp overflows to inf for v < -88, s = 0, both finite
template <typename F>
__device__ __forceinline__ F gnc_sigmoid(F v) {
  if constexpr (sizeof(F) == 4) return 1.f / (1.f + expf(-v));
  else return 1.0 / (1.0 + exp(-v));
}
template <typename F>
__device__ __forceinline__ F gnc_silu(F v) {
  return v * gnc_sigmoid<F>(v);
}
template <typename F>
__device__ __forceinline__ F gnc_silu_grad(F v) {
  const F s = gnc_sigmoid<F>(v);
  return s * ((F)1 + v * ((F)1 - s));
}

// ge / be [n_batch][c] (any of gamma / beta [c], scale / shift [n_batch][c] may be NULL: 1 / 0 / 0 / 0)
template <typename F>
__global__ __launch_bounds__(256) void k_gnc_coef(const F *__restrict__ gamma, const F *__restrict__ beta,
                                                 const F *__restrict__ scale, const F *__restrict__ shift, int n_batch,
                                                 int c, F *__restrict__ ge, F *__restrict__ be) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_batch * c) return;
  const int ch = idx % c;
  const F one = (F)1 + (scale != nullptr ? scale[idx] : (F)0);
  ge[idx] = (gamma != nullptr ? gamma[ch] : (F)1) * one;
  be[idx] = fma(beta != nullptr ? beta[ch] : (F)0, one, shift != nullptr ? shift[idx] : (F)0);
}

// the gradient that the partial kernel sums with the SiLU: dv = dy * act'(v), v = (x - mean) * (rstd * ge) + be as the
// forward map forms it; the product is rounded on its own so that the partial kernel and the backward map hold the same
// dv bit for bit
struct GncGrad {
  const float *ge, *be;
  int c;
  template <int V>
  struct State {
    float a[V], be[V];
  };
  template <int V>
  __device__ __forceinline__ void load(int b, int ch0, const float (&rs)[V], State<V> &st) const {
    float g[V];
    load_f32<V>(ge + (int64_t)b * c + ch0, g);
    load_f32<V>(be + (int64_t)b * c + ch0, st.be);
#pragma unroll
    for (int j = 0; j < V; ++j) st.a[j] = rs[j] * g[j];
  }
  template <int V>
  __device__ __forceinline__ float operator()(const State<V> &st, int j, float xc, float g) const {
    return mul_rounded(g, gnc_silu_grad<float>(fmaf(xc, st.a[j], st.be[j])));
  }
};

// ---- the row maps of both group norms (seg_rows, segment_norm.hpp) -------------------------------------------------------
// Where the affine map of (instance, channel) comes from.  BE: whether the additive term is wanted.
// per channel: gamma / beta [c] (either may be NULL: 1 / 0), loaded once per piece, outside the row loop
struct GnPerChannel {
  const float *gamma, *beta;
  template <int V, bool BE>
  __device__ __forceinline__ void init(int ch0, float (&ga)[V], float (&be)[V]) const {
    load_affine<V>(gamma, BE ? beta : nullptr, ch0, ga, be);
  }
  template <int V, bool BE>
  __device__ __forceinline__ void load(int, int, float (&)[V], float (&)[V]) const {}
  const float *weight() const { return gamma; }   // of k_gn_bwd_group
  int weight_stride() const { return 0; }
};
// per (instance, channel): ge / be [n_batch][c] (k_gnc_coef), loaded at a change of the batch index
struct GnPerInstance {
  const float *ge, *be;
  int c;
  template <int V, bool BE>
  __device__ __forceinline__ void init(int, float (&)[V], float (&)[V]) const {}
  template <int V, bool BE>
  __device__ __forceinline__ void load(int b, int ch0, float (&ga)[V], float (&bev)[V]) const {
    load_f32<V>(ge + (int64_t)b * c + ch0, ga);
    if constexpr (BE) load_f32<V>(be + (int64_t)b * c + ch0, bev);
  }
  const float *weight() const { return ge; }
  int weight_stride() const { return c; }
};

// y = act((x - mean[b, g]) * (rstd[b, g] * ga) + be), ga / be from Aff; the activation in fp32, one rounding at a bf16
// store.  A thread's piece may straddle groups (cg = 3 with 4 floats, cg = 6 with 8 bf16): the group of every element is
// computed once per piece.  mean / rstd are read element by element ([n_batch, groups] floats, L2-resident, no alignment
// asked of them).
template <typename Aff, int ACT>
struct GnFwd {
  static constexpr bool kDy = false;
  const float *mean, *rstd;
  Aff aff;
  int groups, cg;
  template <int V>
  struct Piece {
    float ga[V], be[V], a[V], mu[V];
    int grp[V];
  };
  template <int V>
  __device__ __forceinline__ void init(int ch0, Piece<V> &pc) const {
    aff.template init<V, true>(ch0, pc.ga, pc.be);
    gn_piece_groups<V>(ch0, cg, pc.grp);
  }
  template <int V>
  __device__ __forceinline__ void load(int b, int ch0, Piece<V> &pc) const {
    aff.template load<V, true>(b, ch0, pc.ga, pc.be);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int o = b * groups + pc.grp[j];
      pc.mu[j] = mean[o];
      pc.a[j] = rstd[o] * pc.ga[j];
    }
  }
  template <int V>
  __device__ __forceinline__ float value(const Piece<V> &pc, int j, float x) const {
    const float v = fmaf(x - pc.mu[j], pc.a[j], pc.be[j]);
    return ACT == kGncSilu ? gnc_silu<float>(v) : v;
  }
};

// dx = A * ((ga * dv - k1) - (x - mean[b, g]) * k2) with A = rstd[b, g], k1 = T1[b, g] / m, k2 = T2[b, g] / m * A,
// m = n_b * cg and dv = dy * act'(v).  ga * dv is rounded on its own: with one value per (instance, group) it equals k1
// bit for bit and dx is exactly 0, which a contraction into one fma would lose.  be and a = A * ga serve the SiLU only.
template <typename Aff, int ACT>
struct GnBwd {
  static constexpr bool kDy = true;
  const float *mean, *rstd;
  Aff aff;
  const float *g1, *g2, *rows;
  int groups, cg;
  template <int V>
  struct Piece {
    float ga[V], be[V], a[V], A[V], k1[V], k2[V], mu[V];
    int grp[V];
  };
  template <int V>
  __device__ __forceinline__ void init(int ch0, Piece<V> &pc) const {
    aff.template init<V, ACT == kGncSilu>(ch0, pc.ga, pc.be);
    gn_piece_groups<V>(ch0, cg, pc.grp);
  }
  template <int V>
  __device__ __forceinline__ void load(int b, int ch0, Piece<V> &pc) const {
    const float inv_m = 1.f / fmaxf(rows[b] * (float)cg, 1.f);
    aff.template load<V, ACT == kGncSilu>(b, ch0, pc.ga, pc.be);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int o = b * groups + pc.grp[j];
      pc.mu[j] = mean[o];
      pc.A[j] = rstd[o];
      if (ACT == kGncSilu) pc.a[j] = pc.A[j] * pc.ga[j];
      pc.k1[j] = g1[o] * inv_m;
      pc.k2[j] = g2[o] * inv_m * pc.A[j];
    }
  }
  template <int V>
  __device__ __forceinline__ float value(const Piece<V> &pc, int j, float x, float dy) const {
    const float xc = x - pc.mu[j];
    float dv = dy;
    if (ACT == kGncSilu) dv = mul_rounded(dv, gnc_silu_grad<float>(fmaf(xc, pc.a[j], pc.be[j])));
    return pc.A[j] * ((mul_rounded(pc.ga[j], dv) - pc.k1[j]) - xc * pc.k2[j]);
  }
  // what the partial kernel sums for this map
  auto grad() const {
    if constexpr (ACT == kGncSilu) return GncGrad{aff.ge, aff.be, aff.c};
    else return SegGradPlain{};
  }
};

// One thread per channel, the instances ascending.  Every requested word is written; an instance without rows on this
// map has t1 = t2 = 0 (seg_bwd_final), so its rows of grad_scale / grad_shift are exactly 0.
template <typename F>
__global__ __launch_bounds__(256) void k_gnc_bwd_params(const F *__restrict__ t1, const F *__restrict__ t2,
                                                       const F *__restrict__ gamma, const F *__restrict__ beta,
                                                       const F *__restrict__ scale, int n_batch, int c,
                                                       F *__restrict__ grad_gamma, F *__restrict__ grad_beta,
                                                       F *__restrict__ grad_scale, F *__restrict__ grad_shift) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const F ga = gamma != nullptr ? gamma[ch] : (F)1, be = beta != nullptr ? beta[ch] : (F)0;
  F a = 0, q = 0;
  for (int b = 0; b < n_batch; ++b) {
    const int64_t o = (int64_t)b * c + ch;
    const F one = (F)1 + (scale != nullptr ? scale[o] : (F)0);
    const F u1 = t1[o], u2 = t2[o];
    a = fma(one, u1, a);
    q = fma(one, u2, q);
    if (grad_shift != nullptr) grad_shift[o] = u1;
    if (grad_scale != nullptr) grad_scale[o] = fma(ga, u2, be * u1);
  }
  if (grad_beta != nullptr) grad_beta[ch] = a;
  if (grad_gamma != nullptr) grad_gamma[ch] = q;
}

// ---- float64 twins: plain double, one thread per output -----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gnc_apply_f64(const double *__restrict__ x,
                                                      const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                      int n_batch, int groups, const double *__restrict__ mean,
                                                      const double *__restrict__ rstd, const double *__restrict__ gamma,
                                                      const double *__restrict__ beta, const double *__restrict__ scale,
                                                      const double *__restrict__ shift, int act,
                                                      double *__restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * c) return;
  const int ch = (int)(idx % c);
  const int b = min(max(batch_row[idx / c], 0), n_batch - 1);
  const int o = b * groups + ch / (c / groups);
  const int64_t e = (int64_t)b * c + ch;
  const double one = 1.0 + (scale ? scale[e] : 0.0);
  const double ge = (gamma ? gamma[ch] : 1.0) * one, be = fma(beta ? beta[ch] : 0.0, one, shift ? shift[e] : 0.0);
  const double v = fma((x[idx] - mean[o]) * rstd[o], ge, be);
  y[idx] = act == kGncSilu ? gnc_silu<double>(v) : v;
}

// t1[b, c] = sum dv, t2[b, c] = sum dv * xhat, rows[b]
__global__ __launch_bounds__(256) void k_gnc_bwd_sums_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                         const int32_t *__restrict__ batch_row, int64_t n, int n_batch,
                                                         int c, int groups, const double *__restrict__ mean,
                                                         const double *__restrict__ rstd, const double *__restrict__ ge,
                                                         const double *__restrict__ be, int act,
                                                         double *__restrict__ t1, double *__restrict__ t2,
                                                         double *__restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_batch * c) return;
  const int b = (int)(idx / c), ch = (int)(idx % c);
  const double m = mean[b * groups + ch / (c / groups)], rs = rstd[b * groups + ch / (c / groups)];
  const double w = ge[idx], o = be[idx];
  double a = 0.0, q = 0.0, cnt = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    if (batch_row[r] != b) continue;
    const double xh = (x[r * c + ch] - m) * rs;
    double g = dy[r * c + ch];
    if (act == kGncSilu) g *= gnc_silu_grad<double>(fma(xh, w, o));
    a += g;
    q = fma(g, xh, q);
    cnt += 1.0;
  }
  t1[idx] = a;
  t2[idx] = q;
  if (ch == 0) rows[b] = cnt;
}

__global__ __launch_bounds__(256) void k_gnc_bwd_apply_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                          const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                          int n_batch, int groups, const double *__restrict__ mean,
                                                          const double *__restrict__ rstd, const double *__restrict__ ge,
                                                          const double *__restrict__ be, int act,
                                                          const double *__restrict__ g1, const double *__restrict__ g2,
                                                          const double *__restrict__ rows, double *__restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * c) return;
  const int ch = (int)(idx % c);
  const int b = min(max(batch_row[idx / c], 0), n_batch - 1);
  const int o = b * groups + ch / (c / groups);
  const int64_t e = (int64_t)b * c + ch;
  const double inv_m = 1.0 / fmax(rows[b] * (double)(c / groups), 1.0);
  const double xh = (x[idx] - mean[o]) * rstd[o];
  double dv = dy[idx];
  if (act == kGncSilu) dv *= gnc_silu_grad<double>(fma(xh, ge[e], be[e]));
  dx[idx] = rstd[o] * (ge[e] * dv - g1[o] * inv_m - xh * g2[o] * inv_m);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// workspace: in_ws_layout_f32 | g1 | g2 [n_batch][groups] floats.  The statistics keep the channel records in t1 / t2.
// float64: t1 | t2 [n_batch][c] | rows [n_batch] | g1 | g2 [n_batch][groups] doubles.  Every piece 256-byte aligned.
struct GnWs {
  InWs in;
  float *g1, *g2;
};
struct GnWs64 {
  double *t1, *t2, *rows, *g1, *g2;
};
static int64_t gn_ws_layout(int64_t n, int n_batch, int c, int groups, char *base, GnWs *w, GnWs64 *w64) {
  const int64_t in32 = in_ws_layout_f32(n, n_batch, c, base, w != nullptr ? &w->in : nullptr);
  const int64_t gs = align_up((int64_t)n_batch * groups * 4, 256);
  if (w != nullptr) {
    w->g1 = reinterpret_cast<float *>(base + in32);
    w->g2 = reinterpret_cast<float *>(base + in32 + gs);
  }
  const int64_t t = align_up((int64_t)n_batch * c * 8, 256), rw = align_up((int64_t)n_batch * 8, 256);
  const int64_t gs64 = align_up((int64_t)n_batch * groups * 8, 256);
  if (w64 != nullptr) {
    w64->t1 = reinterpret_cast<double *>(base);
    w64->t2 = reinterpret_cast<double *>(base + t);
    w64->rows = reinterpret_cast<double *>(base + 2 * t);
    w64->g1 = reinterpret_cast<double *>(base + 2 * t + rw);
    w64->g2 = reinterpret_cast<double *>(base + 2 * t + rw + gs64);
  }
  const int64_t f32 = in32 + 2 * gs, f64 = 2 * t + rw + 2 * gs64;
  return f32 > f64 ? f32 : f64;
}

// ---- host side: the group-norm workspace, then ge | be [n_batch][c] (floats, or doubles for the _f64 entry points) ------
struct GncWs {
  GnWs w;
  GnWs64 w64;
  char *ge, *be;
};
static int64_t gnc_ws_layout(int64_t n, int n_batch, int c, int groups, char *base, GncWs *w) {
  const int64_t gn = align_up(gn_ws_layout(n, n_batch, c, groups, base, w != nullptr ? &w->w : nullptr,
                                           w != nullptr ? &w->w64 : nullptr), 256);
  const int64_t co = align_up((int64_t)n_batch * c * 8, 256);
  if (w != nullptr) {
    w->ge = base + gn;
    w->be = base + gn + co;
  }
  return gn + 2 * co;
}

#define ME_GNC_DISPATCH_ACT(act, ...)                               \
  do {                                                              \
    if ((act) == kGncSilu) { constexpr int ACT = kGncSilu; __VA_ARGS__; } \
    else { constexpr int ACT = kGncIdentity; __VA_ARGS__; }         \
  } while (0)

template <typename F>
static void gnc_coef(const F *gamma, const F *beta, const F *scale, const F *shift, int n_batch, int c, const GncWs &w,
                     hipStream_t stream) {
  hipLaunchKernelGGL(k_gnc_coef<F>, dim3((unsigned)ceil_div((int64_t)n_batch * c, 256)), dim3(256), 0, stream, gamma, beta,
                     scale, shift, n_batch, c, reinterpret_cast<F *>(w.ge), reinterpret_cast<F *>(w.be));
}

template <typename T>
static int gn_stats(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, int groups, float eps,
                    float *mean, float *rstd, const GnWs &w, hipStream_t stream) {
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread, {x});
  ME_CHECK(pl.lds <= 64 * 1024, "channel count too large for the group-norm kernels");
  ME_HIP(hipMemsetAsync(w.in.cnt, 0, (size_t)pl.chunks * n_batch * 4, stream));
  if (n > 0)
    ME_PIECE_DISPATCH(T, kPieceNorm, pl.v,
                      hipLaunchKernelGGL((k_gn_partial<T, V>), dim3(pl.chunks), dim3(256), pl.lds, stream, x, batch_row, n,
                                         c, pl.chunks, n_batch, w.in.pa, w.in.pb, w.in.cnt));
  hipLaunchKernelGGL(k_gn_chan_final, dim3((unsigned)ceil_div((int64_t)n_batch * c, 4)), dim3(256), 0, stream, w.in.pa,
                     w.in.pb, w.in.cnt, pl.chunks, n_batch, c, w.in.t1, w.in.t2, w.in.rows);
  hipLaunchKernelGGL(k_gn_group_final, dim3((unsigned)ceil_div((int64_t)n_batch * groups, 256)), dim3(256), 0, stream,
                     w.in.t1, w.in.t2, w.in.rows, n_batch, c, groups, eps, mean, rstd);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int gn_apply(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, int groups, const float *mean,
                    const float *rstd, const float *gamma, const float *beta, T *y, hipStream_t stream) {
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread, {x, y});
  const GnFwd<GnPerChannel, kGncIdentity> map{mean, rstd, {gamma, beta}, groups, c / groups};
  ME_SEG_ROWS(T, pl, stream, x, (const T *)nullptr, batch_row, n, c, n_batch, map, y);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int gnc_apply(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, int groups, const float *mean,
                     const float *rstd, const float *gamma, const float *beta, const float *scale, const float *shift,
                     int act, T *y, const GncWs &w, hipStream_t stream) {
  const float *ge = reinterpret_cast<const float *>(w.ge), *be = reinterpret_cast<const float *>(w.be);
  gnc_coef<float>(gamma, beta, scale, shift, n_batch, c, w, stream);
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread, {x, y});
  ME_GNC_DISPATCH_ACT(act, const GnFwd<GnPerInstance, ACT> map{mean, rstd, {ge, be, c}, groups, c / groups};
                      ME_SEG_ROWS(T, pl, stream, x, (const T *)nullptr, batch_row, n, c, n_batch, map, y));
  ME_LAUNCH_CHECK();
  return 0;
}

// The backward launches of both group norms, from the backward map `map` (GnBwd): its gradient for the partial kernel, its
// affine source as the weights of k_gn_bwd_group.  gamma / beta / scale: k_gnc_bwd_params' (NULL: 1 / 0 / 0).
template <typename T, typename Map>
static int gn_backward_run(const T *x, const T *dy, const int32_t *batch_row, int64_t n, int n_batch, int c,
                           const Map &map, const float *gamma, const float *beta, const float *scale, T *dx,
                           float *grad_gamma, float *grad_beta, float *grad_scale, float *grad_shift, const GnWs &w,
                           hipStream_t stream) {
  const SegPlan pl = seg_plan<T>(n, c, kBnRowsPerThread / 2, {x, dy, dx});
  ME_CHECK(pl.lds <= 64 * 1024, "channel count too large for the group-norm kernels");
  ME_HIP(hipMemsetAsync(w.in.cnt, 0, (size_t)pl.chunks * n_batch * 4, stream));
  const auto grad = map.grad();
  const GnCoef coef{map.mean, map.rstd, map.groups, map.cg};
  ME_PIECE_DISPATCH(T, kPieceNorm, pl.v,
                    hipLaunchKernelGGL((k_gn_bwd_partial<T, V, std::decay_t<decltype(grad)>>), dim3(pl.chunks), dim3(256),
                                       pl.lds, stream, x, dy, batch_row, n, c, pl.chunks, n_batch, coef, grad, w.in.pa,
                                       w.in.pb, w.in.cnt));
  hipLaunchKernelGGL(k_gn_bwd_final, dim3((unsigned)ceil_div((int64_t)n_batch * c, 4)), dim3(256), 0, stream, w.in.pa,
                     w.in.pb, w.in.cnt, pl.chunks, n_batch, c, w.in.t1, w.in.t2, w.in.rows);
  if (grad_gamma != nullptr || grad_beta != nullptr || grad_scale != nullptr || grad_shift != nullptr)
    hipLaunchKernelGGL(k_gnc_bwd_params<float>, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, stream, w.in.t1, w.in.t2,
                       gamma, beta, scale, n_batch, c, grad_gamma, grad_beta, grad_scale, grad_shift);
  if (dx != nullptr) {
    hipLaunchKernelGGL(k_gn_bwd_group<float>, dim3((unsigned)ceil_div((int64_t)n_batch * map.groups, 256)), dim3(256), 0,
                       stream, w.in.t1, w.in.t2, map.aff.weight(), map.aff.weight_stride(), n_batch, c, map.groups, w.g1,
                       w.g2);
    ME_SEG_ROWS(T, pl, stream, x, dy, batch_row, n, c, n_batch, map, dx);
  }
  ME_LAUNCH_CHECK();
  return 0;
}

// plain group norm: grad_beta = sum_b t1 and grad_gamma = sum_b t2 are k_gnc_bwd_params' sums without modulation
// (fma(1, u, a) is a + u)
template <typename T>
static int gn_backward(const T *x, const T *dy, const int32_t *batch_row, int64_t n, int n_batch, int c, int groups,
                       const float *mean, const float *rstd, const float *gamma, T *dx, float *grad_gamma,
                       float *grad_beta, const GnWs &w, hipStream_t stream) {
  const GnBwd<GnPerChannel, kGncIdentity> map{mean, rstd, {gamma, nullptr}, w.g1, w.g2, w.in.rows, groups, c / groups};
  return gn_backward_run<T>(x, dy, batch_row, n, n_batch, c, map, nullptr, nullptr, nullptr, dx, grad_gamma, grad_beta,
                            nullptr, nullptr, w, stream);
}

template <typename T>
static int gnc_backward(const T *x, const T *dy, const int32_t *batch_row, int64_t n, int n_batch, int c, int groups,
                        const float *mean, const float *rstd, const float *gamma, const float *beta, const float *scale,
                        const float *shift, int act, T *dx, float *grad_gamma, float *grad_beta, float *grad_scale,
                        float *grad_shift, const GncWs &ws, hipStream_t stream) {
  const GnWs &w = ws.w;
  const float *ge = reinterpret_cast<const float *>(ws.ge), *be = reinterpret_cast<const float *>(ws.be);
  gnc_coef<float>(gamma, beta, scale, shift, n_batch, c, ws, stream);
  ME_GNC_DISPATCH_ACT(act, const GnBwd<GnPerInstance, ACT> map{mean, rstd, {ge, be, c}, w.g1, w.g2, w.in.rows, groups,
                                                               c / groups};
                      return gn_backward_run<T>(x, dy, batch_row, n, n_batch, c, map, gamma, beta, scale, dx, grad_gamma,
                                                grad_beta, grad_scale, grad_shift, w, stream));
}

}  // namespace me

using namespace me;

// host-only argument checks: nothing is launched when one fails
#define ME_GN_CHECK_ARGS()                                                                                       \
  ME_CHECK(n >= 0 && c > 0 && n_batch > 0, "group norm needs a channel count and at least one instance");        \
  ME_CHECK(groups > 0 && c % groups == 0, "group norm: the channel count must be a multiple of the groups");     \
  ME_CHECK(n < (1ll << 40) && (int64_t)n_batch * c < (1ll << 31), "group norm: matrix or statistics too large")
// the partial kernels' LDS with one row lane (5 c + 256 floats): rows of up to 3225 channels
#define ME_GN_CHECK_WIDTH() \
  ME_CHECK(in_partial_lds_bytes(c, 1) <= 64 * 1024, "channel count too large for the group-norm kernels")

extern "C" {

int64_t me_gnorm_workspace_bytes(int64_t n, int32_t n_batch, int32_t c, int32_t groups) {
  if (n_batch <= 0 || c <= 0 || groups <= 0) return 0;
  return gn_ws_layout(n < 0 ? 0 : n, n_batch, c, groups, nullptr, nullptr, nullptr);
}

int me_gnorm_stats(const void *x, int32_t is_bf16, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                   int32_t groups, float eps, float *mean, float *rstd, void *workspace, int64_t workspace_bytes,
                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_GN_CHECK_WIDTH();
  ME_CHECK(workspace_bytes >= me_gnorm_workspace_bytes(n, n_batch, c, groups), "workspace too small");
  GnWs w;
  gn_ws_layout(n, n_batch, c, groups, reinterpret_cast<char *>(workspace), &w, nullptr);
  ME_SEG_RETURN_T(is_bf16, gn_stats<T>((const T *)x, batch_row, n, n_batch, c, groups, eps, mean, rstd, w, stream));
}

int me_gnorm_apply(const void *x, int32_t is_bf16, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                   int32_t groups, const float *mean, const float *rstd, const float *gamma, const float *beta, void *y,
                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_GN_CHECK_WIDTH();
  if (n == 0) return 0;
  ME_SEG_RETURN_T(is_bf16, gn_apply<T>((const T *)x, batch_row, n, n_batch, c, groups, mean, rstd, gamma, beta, (T *)y,
                                       stream));
}

int me_gnorm_backward(const void *x, const void *dy, int32_t is_bf16, const int32_t *batch_row, int64_t n,
                      int32_t n_batch, int32_t c, int32_t groups, const float *mean, const float *rstd,
                      const float *gamma, void *dx, float *grad_gamma, float *grad_beta, void *workspace,
                      int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_GN_CHECK_WIDTH();
  ME_CHECK(n > 0, "group norm backward needs at least one row");
  ME_CHECK(workspace_bytes >= me_gnorm_workspace_bytes(n, n_batch, c, groups), "workspace too small");
  GnWs w;
  gn_ws_layout(n, n_batch, c, groups, reinterpret_cast<char *>(workspace), &w, nullptr);
  ME_SEG_RETURN_T(is_bf16, gn_backward<T>((const T *)x, (const T *)dy, batch_row, n, n_batch, c, groups, mean, rstd, gamma,
                                          (T *)dx, grad_gamma, grad_beta, w, stream));
}

int me_gnorm_stats_f64(const double *x, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c, int32_t groups,
                       double eps, double *mean, double *rstd, void *stream_) {
  ME_GN_CHECK_ARGS();
  hipLaunchKernelGGL(k_gn_stats_f64, dim3((unsigned)ceil_div((int64_t)n_batch * groups, 256)), dim3(256), 0,
                     (hipStream_t)stream_, x, batch_row, n, n_batch, c, groups, eps, mean, rstd);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_gnorm_apply_f64(const double *x, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c, int32_t groups,
                       const double *mean, const double *rstd, const double *gamma, const double *beta, double *y,
                       void *stream_) {
  ME_GN_CHECK_ARGS();
  if (n == 0) return 0;
  // the conditional twin without modulation: gamma * 1.0 and fma(beta, 1.0, 0.0) are exact
  hipLaunchKernelGGL(k_gnc_apply_f64, dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, (hipStream_t)stream_, x,
                     batch_row, n, c, n_batch, groups, mean, rstd, gamma, beta, (const double *)nullptr,
                     (const double *)nullptr, (int)kGncIdentity, y);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_gnorm_backward_f64(const double *x, const double *dy, const int32_t *batch_row, int64_t n, int32_t n_batch,
                          int32_t c, int32_t groups, const double *mean, const double *rstd, const double *gamma,
                          double *dx, double *grad_gamma, double *grad_beta, void *workspace, int64_t workspace_bytes,
                          void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_CHECK(workspace_bytes >= me_gnorm_workspace_bytes(n, n_batch, c, groups), "workspace too small");
  GnWs64 w;
  gn_ws_layout(n, n_batch, c, groups, reinterpret_cast<char *>(workspace), nullptr, &w);
  hipLaunchKernelGGL(k_gn_bwd_sums_f64, dim3((unsigned)ceil_div((int64_t)n_batch * c, 256)), dim3(256), 0, stream, x, dy,
                     batch_row, n, n_batch, c, groups, mean, rstd, w.t1, w.t2, w.rows);
  if (grad_gamma != nullptr || grad_beta != nullptr)
    hipLaunchKernelGGL(k_gnc_bwd_params<double>, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, stream, w.t1, w.t2,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, n_batch, c, grad_gamma,
                       grad_beta, (double *)nullptr, (double *)nullptr);
  if (dx != nullptr && n > 0) {
    hipLaunchKernelGGL(k_gn_bwd_group<double>, dim3((unsigned)ceil_div((int64_t)n_batch * groups, 256)), dim3(256), 0,
                       stream, w.t1, w.t2, gamma, 0, n_batch, c, groups, w.g1, w.g2);
    hipLaunchKernelGGL(k_gn_bwd_apply_f64, dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, stream, x, dy, batch_row, n,
                       c, n_batch, groups, mean, rstd, gamma, w.g1, w.g2, w.rows, dx);
  }
  ME_LAUNCH_CHECK();
  return 0;
}

// ---- conditional group norm ---------------------------------------------------------------------------------------------
#define ME_GNC_CHECK_ACT() ME_CHECK(act == kGncIdentity || act == kGncSilu, "conditional group norm: act must be 0 (identity) or 1 (SiLU)")

int64_t me_gnorm_cond_workspace_bytes(int64_t n, int32_t n_batch, int32_t c, int32_t groups) {
  if (n_batch <= 0 || c <= 0 || groups <= 0) return 0;
  return gnc_ws_layout(n < 0 ? 0 : n, n_batch, c, groups, nullptr, nullptr);
}

int me_gnorm_cond_apply(const void *x, int32_t is_bf16, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                        int32_t groups, const float *mean, const float *rstd, const float *gamma, const float *beta,
                        const float *scale, const float *shift, int32_t act, void *y, void *workspace,
                        int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_GNC_CHECK_ACT();
  ME_GN_CHECK_WIDTH();
  ME_CHECK(workspace_bytes >= me_gnorm_cond_workspace_bytes(n, n_batch, c, groups), "workspace too small");
  if (n == 0) return 0;
  GncWs w;
  gnc_ws_layout(n, n_batch, c, groups, reinterpret_cast<char *>(workspace), &w);
  ME_SEG_RETURN_T(is_bf16, gnc_apply<T>((const T *)x, batch_row, n, n_batch, c, groups, mean, rstd, gamma, beta, scale,
                                        shift, act, (T *)y, w, stream));
}

int me_gnorm_cond_backward(const void *x, const void *dy, int32_t is_bf16, const int32_t *batch_row, int64_t n,
                           int32_t n_batch, int32_t c, int32_t groups, const float *mean, const float *rstd,
                           const float *gamma, const float *beta, const float *scale, const float *shift, int32_t act,
                           void *dx, float *grad_gamma, float *grad_beta, float *grad_scale, float *grad_shift,
                           void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_GNC_CHECK_ACT();
  ME_GN_CHECK_WIDTH();
  ME_CHECK(n > 0, "group norm backward needs at least one row");
  ME_CHECK(workspace_bytes >= me_gnorm_cond_workspace_bytes(n, n_batch, c, groups), "workspace too small");
  GncWs w;
  gnc_ws_layout(n, n_batch, c, groups, reinterpret_cast<char *>(workspace), &w);
  ME_SEG_RETURN_T(is_bf16, gnc_backward<T>((const T *)x, (const T *)dy, batch_row, n, n_batch, c, groups, mean, rstd,
                                           gamma, beta, scale, shift, act, (T *)dx, grad_gamma, grad_beta, grad_scale,
                                           grad_shift, w, stream));
}

int me_gnorm_cond_apply_f64(const double *x, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                            int32_t groups, const double *mean, const double *rstd, const double *gamma,
                            const double *beta, const double *scale, const double *shift, int32_t act, double *y,
                            void *stream_) {
  ME_GN_CHECK_ARGS();
  ME_GNC_CHECK_ACT();
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_gnc_apply_f64, dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, (hipStream_t)stream_, x,
                     batch_row, n, c, n_batch, groups, mean, rstd, gamma, beta, scale, shift, act, y);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_gnorm_cond_backward_f64(const double *x, const double *dy, const int32_t *batch_row, int64_t n, int32_t n_batch,
                               int32_t c, int32_t groups, const double *mean, const double *rstd, const double *gamma,
                               const double *beta, const double *scale, const double *shift, int32_t act, double *dx,
                               double *grad_gamma, double *grad_beta, double *grad_scale, double *grad_shift,
                               void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_GN_CHECK_ARGS();
  ME_GNC_CHECK_ACT();
  ME_CHECK(workspace_bytes >= me_gnorm_cond_workspace_bytes(n, n_batch, c, groups), "workspace too small");
  GncWs ws;
  gnc_ws_layout(n, n_batch, c, groups, reinterpret_cast<char *>(workspace), &ws);
  const GnWs64 &w = ws.w64;
  const double *ge = reinterpret_cast<const double *>(ws.ge), *be = reinterpret_cast<const double *>(ws.be);
  gnc_coef<double>(gamma, beta, scale, shift, n_batch, c, ws, stream);
  hipLaunchKernelGGL(k_gnc_bwd_sums_f64, dim3((unsigned)ceil_div((int64_t)n_batch * c, 256)), dim3(256), 0, stream, x, dy,
                     batch_row, n, n_batch, c, groups, mean, rstd, ge, be, act, w.t1, w.t2, w.rows);
  if (grad_gamma != nullptr || grad_beta != nullptr || grad_scale != nullptr || grad_shift != nullptr)
    hipLaunchKernelGGL(k_gnc_bwd_params<double>, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, stream, w.t1, w.t2,
                       gamma, beta, scale, n_batch, c, grad_gamma, grad_beta, grad_scale, grad_shift);
  if (dx != nullptr && n > 0) {
    hipLaunchKernelGGL(k_gn_bwd_group<double>, dim3((unsigned)ceil_div((int64_t)n_batch * groups, 256)), dim3(256), 0,
                       stream, w.t1, w.t2, ge, c, n_batch, c, groups, w.g1, w.g2);
    hipLaunchKernelGGL(k_gnc_bwd_apply_f64, dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, stream, x, dy, batch_row,
                       n, c, n_batch, groups, mean, rstd, ge, be, act, w.g1, w.g2, w.rows, dx);
  }
  ME_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_group_norm(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::k_gn_chan_final));
}
