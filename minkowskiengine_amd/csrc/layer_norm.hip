// Layer norm and RMS norm over the channel axis of a feature matrix [n, c] for gfx950 (MI355X), with the residual add of a
// pre-norm block folded in (MinkowskiLayerNorm, MinkowskiRMSNorm; definition in include/me_amd.h, ABI 1.23).  Row-local:
// no coordinate map, one pass over the matrix forward, one pass plus a small merge backward.
//
//   * Row teams.  A row lives in the registers of a team of L lanes (L = 1 .. 64, a power of two), P pieces of V channels
//     per lane: piece q = p * L + lane holds the channels [q V, q V + V), so the lanes of a team read consecutive 16 bytes.
//     L * P * V >= c; a piece past the row reads piece 0 and is zeroed, a team past the matrix reads the last row and
//     stores nothing.  Small rows share a wave (bf16 c = 64: 8 lanes a row, 8 rows a wave); (L, P) is chosen on the host.
//   * Sums over a row are ONE balanced tree over the channel index padded with zeros to L * P * V: inside a piece, then
//     over the lanes of the team by xor exchanges of distance 1, 2, .. L / 2 (never beyond the team: a NaN stays in its
//     row), then over p.  Zeros add exactly, so the tree — and every bit of y, stream, dx — is the same for every (V, L, P)
//     that can serve a row: an aligned matrix, a column view and a misaligned view give the same bits.
//   * k_ln_forward: [stream = T(float(residual) + float(x)), stored,] the mean from sum(x - x[0]) (layer norm does not
//     change when a row is shifted, the differences of close values are exact, and a constant row is centred to exactly
//     0), the centred sum of squares from the registers, rstd, the affine map, one rounded store.  RMS: no mean,
//     rstd = 1 / sqrt(sum(x^2) / c + eps); rstd is rounded once (rsqrt_rn).  gamma / beta are loaded once per lane before a persistent row loop.
//   * k_ln_backward: workgroup g owns the rows [chunk_begin(g), chunk_begin(g + 1)).  Per row xhat (the row centred again
//     as in the forward pass — one more butterfly, no traffic — not on the saved fp32 mean, whose rounding is large against a
//     small deviation), g = dy gamma, s1 = sum g,
//     s2 = sum g xhat, dx = rstd ((g - s1 / c) - xhat s2 / c) (RMS: without s1; the product is not rounded on its own,
//     and s2 and xhat carry the remainders of their roundings: three butterflies for the layer norm, two for RMS), rounded to T, + dstream (rounded again, as the
//     gradient accumulation of the unfused graph rounds), one store.  Each lane adds dy xhat (xhat with the part its rounding lost: dy d rstd
//     is rounded once) and dy of its channels over
//     its rows in ascending order; the teams of a wave are combined by xor exchanges across the team index, the waves
//     through LDS in wave order, and one [2][c] record leaves the workgroup.  k_ln_param_reduce sums the G records per
//     channel in ascending g.  No atomics; G is a pure function of (n, c, element size).
//   * The float64 twins are the plain formulas, one wave a row and one thread a channel: the gradcheck yardstick.
// Byte model: forward 2 n c e (4 n c e with the residual), backward 3 n c e.
// The team helpers (exchanges, the tree, centre, rsqrt_rn, the (L, P) dispatch) are row_team.hpp, shared with
// ada_layer_norm.hip.
#include "row_team.hpp"

namespace me {
namespace lnorm {

struct ForwardArgs {
  const void *x, *res;
  void *sout, *y;
  int64_t xs, rs, ss, ys, n;
  int c, iters;
  const float *gamma, *beta;
  float eps;
  float *mean, *rstd;
};

template <typename T, int V, int L, int P, bool RMS>
__global__ __launch_bounds__(kThreads) void k_ln_forward(const ForwardArgs a) {
  constexpr int R = kThreads / L;   // rows of a workgroup per step
  const T *x = (const T *)a.x, *res = (const T *)a.res;
  T *sout = (T *)a.sout, *y = (T *)a.y;
  const int team = threadIdx.x / L;
  const float fc = (float)a.c;
  int ch[P];
  bool ok[P];
  lane_pieces<V, L, P>(a.c, ch, ok);
  float ga[P][V], be[P][V];
  load_param<V, P>(a.gamma, ch, 1.f, ga);
  load_param<V, P>(a.beta, ch, 0.f, be);
  for (int it = 0; it < a.iters; ++it) {
    const int64_t row = ((int64_t)it * gridDim.x + blockIdx.x) * R + team;
    const bool live = row < a.n;
    const int64_t r = live ? row : a.n - 1;
    float xv[P][V];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Piece<V> t = load_piece<T, V>(x + r * a.xs + ch[p]);
      if (res != nullptr) {
        const Piece<V> u = load_piece<T, V>(res + r * a.rs + ch[p]);
#pragma unroll
        for (int j = 0; j < V; ++j) t.v[j] = (float)(T)(u.v[j] + t.v[j]);
        if (live && ok[p]) store_piece<T, V>(sout + r * a.ss + ch[p], t);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) xv[p][j] = ok[p] ? t.v[j] : 0.f;
    }
    float mu = 0.f, d[P][V], sq[P][V];
    if constexpr (!RMS) {
      mu = centre<L, P, V>(xv, ok, fc, d, sq);
    } else {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < V; ++j) d[p][j] = xv[p][j];
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int j = 0; j < V; ++j) sq[p][j] = d[p][j] * d[p][j];
    const float rs = rsqrt_rn(team_sum<L, P, V>(sq) / fc + a.eps);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Piece<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = __builtin_fmaf(d[p][j] * rs, ga[p][j], be[p][j]);
      if (live && ok[p]) store_piece<T, V>(y + r * a.ys + ch[p], o);
    }
    if (live && threadIdx.x % L == 0) {
      if constexpr (!RMS) a.mean[row] = mu;
      a.rstd[row] = rs;
    }
  }
}

struct BackwardArgs {
  const void *x, *dy, *dstream;
  void *dx;
  int64_t xs, dys, dss, dxs, n;
  int c, chunks;
  const float *gamma, *mean, *rstd;
  float *partial;   // [chunks][2][c]: sums of dy xhat and of dy over the rows of a chunk, or NULL
};

template <typename T, int V, int L, int P, bool RMS>
__global__ __launch_bounds__(kThreads) void k_ln_backward(const BackwardArgs a) {
  constexpr int R = kThreads / L;
  __shared__ float red[kThreads / kWave - 1][L * P * V];
  const T *x = (const T *)a.x, *dy = (const T *)a.dy, *dstream = (const T *)a.dstream;
  T *dx = (T *)a.dx;
  const int team = threadIdx.x / L;
  const float fc = (float)a.c;
  int ch[P];
  bool ok[P];
  lane_pieces<V, L, P>(a.c, ch, ok);
  float ga[P][V], ag[P][V], ab[P][V];
  load_param<V, P>(a.gamma, ch, 1.f, ga);
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < V; ++j) ag[p][j] = ab[p][j] = 0.f;
  const int64_t begin = chunk_begin(blockIdx.x, a.n, a.chunks), end = chunk_begin(blockIdx.x + 1, a.n, a.chunks);
  const int64_t last = end > begin ? end - 1 : 0;
  const int iters = (int)((end - begin + R - 1) / R);
  for (int it = 0; it < iters; ++it) {
    const int64_t row = begin + (int64_t)it * R + team;
    const bool live = row < end;
    const int64_t r = live ? row : last;
    const float rs = a.rstd[r];
    float xh[P][V], xe[P][V], dyv[P][V], g[P][V], t1[P][V], t2[P][V];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const Piece<V> xv = load_piece<T, V>(x + r * a.xs + ch[p]);
#pragma unroll
      for (int j = 0; j < V; ++j) t2[p][j] = ok[p] ? xv.v[j] : 0.f;
    }
    // the row is centred again as the forward pass centred it, not on the saved (rounded) mean: xhat has the forward's bits
    if constexpr (!RMS) centre<L, P, V>(t2, ok, fc, xh, t1);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const Piece<V> dv = load_piece<T, V>(dy + r * a.dys + ch[p]);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = RMS ? t2[p][j] : xh[p][j];
        xh[p][j] = d * rs;
        xe[p][j] = __builtin_fmaf(d, rs, -xh[p][j]);   // what the rounding of xhat lost, for the sums of dy xhat
        dyv[p][j] = ok[p] ? dv.v[j] : 0.f;
        t1[p][j] = g[p][j] = dyv[p][j] * ga[p][j];
        t2[p][j] = g[p][j] * xh[p][j];
      }
    }
    const float m1 = RMS ? 0.f : team_sum<L, P, V>(t1) / fc;
    // s2 with what its products lost to rounding (of g xhat, and of xhat itself): where one channel carries a row,
    // g - xhat s2 / c cancels, and those remainders are what is left
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int j = 0; j < V; ++j) t1[p][j] = __builtin_fmaf(g[p][j], xh[p][j], -t2[p][j]) + g[p][j] * xe[p][j];
    const float s2 = team_sum<L, P, V>(t2), s2lo = team_sum<L, P, V>(t1);
    const float m2 = s2 / fc, m2lo = (__builtin_fmaf(-m2, fc, s2) + s2lo) / fc;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Piece<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float t = __builtin_fmaf(-xh[p][j], m2, g[p][j] - m1);
        t = __builtin_fmaf(-xe[p][j], m2, __builtin_fmaf(-xh[p][j], m2lo, t));
        o.v[j] = (float)(T)(t * rs);
      }
      if (dstream != nullptr) {
        const Piece<V> u = load_piece<T, V>(dstream + r * a.dss + ch[p]);
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = o.v[j] + u.v[j];
      }
      if (dx != nullptr && live && ok[p]) store_piece<T, V>(dx + r * a.dxs + ch[p], o);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        ag[p][j] = live ? __builtin_fmaf(dyv[p][j], xh[p][j], __builtin_fmaf(dyv[p][j], xe[p][j], ag[p][j])) : ag[p][j];
        ab[p][j] = live ? ab[p][j] + dyv[p][j] : ab[p][j];
      }
    }
  }
  if (a.partial == nullptr) return;
  // the teams of a wave, then the waves in wave order: first the sums of dy xhat, then those of dy, through one buffer
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float *rec = a.partial + (int64_t)blockIdx.x * 2 * a.c;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    float(&acc)[P][V] = which == 0 ? ag : ab;
#pragma unroll
    for (int p = 0; p < P; ++p) xor_reduce<L, kWave>(acc[p]);
    if (wave > 0 && lane < L) {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < V; ++j) red[wave - 1][(p * L + lane) * V + j] = acc[p][j];
    }
    __syncthreads();
    if (wave == 0 && lane < L) {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float s = acc[p][j];
#pragma unroll
          for (int w = 0; w < kThreads / kWave - 1; ++w) s += red[w][(p * L + lane) * V + j];
          if (ok[p]) rec[which * a.c + ch[p] + j] = s;
        }
    }
    __syncthreads();
  }
}

// grad_gamma[ch] / grad_beta[ch] = the records of the chunks summed in ascending chunk order; chunks = 0 writes zeros
__global__ __launch_bounds__(kThreads) void k_ln_param_reduce(const float *__restrict__ partial, int chunks, int c,
                                                              float *__restrict__ grad_gamma,
                                                              float *__restrict__ grad_beta) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * c) return;
  const int which = idx / c, ch = idx - which * c;
  float *dst = which == 0 ? grad_gamma : grad_beta;
  if (dst == nullptr) return;
  float s = 0.f;
  // (the adds stay in ascending g; unrolled so that 16 loads are in flight instead of one)
#pragma unroll 16
  for (int g = 0; g < chunks; ++g) s += partial[((int64_t)g * 2 + which) * c + ch];
  dst[ch] = s;
}

// ---- float64 twins: one wave a row, the lanes stride over the channels ------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_ln_forward_f64(const double *x, int64_t xs, const double *res, int64_t rs,
                                                             double *sout, int64_t ss, int64_t n, int c, int rms,
                                                             const double *gamma, const double *beta, double eps,
                                                             double *y, int64_t ys, double *mean, double *rstd) {
  const int lane = lane_id();
  const int64_t step = (int64_t)gridDim.x * (kThreads / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; r < n; r += step) {
    double s = 0.0;
    for (int ch = lane; ch < c; ch += kWave) {
      const double v = res != nullptr ? res[r * rs + ch] + x[r * xs + ch] : x[r * xs + ch];
      if (res != nullptr) sout[r * ss + ch] = v;
      s += v;
    }
    const double mu = rms ? 0.0 : wave_sum(s) / c;
    double q = 0.0;
    for (int ch = lane; ch < c; ch += kWave) {
      const double v = (res != nullptr ? res[r * rs + ch] + x[r * xs + ch] : x[r * xs + ch]) - mu;
      q += v * v;
    }
    const double rd = 1.0 / sqrt(wave_sum(q) / c + eps);
    for (int ch = lane; ch < c; ch += kWave) {
      const double v = (res != nullptr ? res[r * rs + ch] + x[r * xs + ch] : x[r * xs + ch]) - mu;
      y[r * ys + ch] = v * rd * (gamma != nullptr ? gamma[ch] : 1.0) + (beta != nullptr ? beta[ch] : 0.0);
    }
    if (lane == 0) {
      if (!rms) mean[r] = mu;
      rstd[r] = rd;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_ln_backward_f64(const double *x, int64_t xs, const double *dy, int64_t dys,
                                                              const double *dstream, int64_t dss, int64_t n, int c, int rms,
                                                              const double *gamma, const double *mean, const double *rstd,
                                                              double *dx, int64_t dxs) {
  const int lane = lane_id();
  const int64_t step = (int64_t)gridDim.x * (kThreads / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; r < n; r += step) {
    const double mu = rms ? 0.0 : mean[r], rd = rstd[r];
    double s1 = 0.0, s2 = 0.0;
    for (int ch = lane; ch < c; ch += kWave) {
      const double g = dy[r * dys + ch] * (gamma != nullptr ? gamma[ch] : 1.0);
      s1 += g;
      s2 += g * ((x[r * xs + ch] - mu) * rd);
    }
    s1 = rms ? 0.0 : wave_sum(s1) / c;
    s2 = wave_sum(s2) / c;
    for (int ch = lane; ch < c; ch += kWave) {
      const double g = dy[r * dys + ch] * (gamma != nullptr ? gamma[ch] : 1.0);
      const double xh = (x[r * xs + ch] - mu) * rd;
      dx[r * dxs + ch] = (g - (s1 + xh * s2)) * rd + (dstream != nullptr ? dstream[r * dss + ch] : 0.0);
    }
  }
}

// one thread a channel, the rows in ascending order
__global__ __launch_bounds__(kThreads) void k_ln_param_f64(const double *x, int64_t xs, const double *dy, int64_t dys,
                                                           int64_t n, int c, int rms, const double *mean,
                                                           const double *rstd, double *grad_gamma, double *grad_beta) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  double sg = 0.0, sb = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    const double d = dy[r * dys + ch];
    sg += d * ((x[r * xs + ch] - (rms ? 0.0 : mean[r])) * rstd[r]);
    sb += d;
  }
  if (grad_gamma != nullptr) grad_gamma[ch] = sg;
  if (grad_beta != nullptr) grad_beta[ch] = sb;
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <typename T, bool RMS>
int forward(ForwardArgs a, hipStream_t stream) {
  const int64_t g = gcd(gcd(gcd(a.c, a.xs), a.ys), gcd(a.res ? a.rs : 0, a.sout ? a.ss : 0));
  const int v = piece_width((int)sizeof(T), (int)g, common_alignment({a.x, a.res, a.sout, a.y, a.gamma, a.beta}),
                            kPieceNorm);
  ME_PIECE_DISPATCH(T, kPieceNorm, v, for_team<V>(a.c / V, [&](auto l, auto p) {
    constexpr int L = decltype(l)::value, P = decltype(p)::value, R = kThreads / L;
    const int64_t blocks = ceil_div(a.n, R) < kMaxBlocks ? ceil_div(a.n, R) : kMaxBlocks;
    a.iters = (int)ceil_div(a.n, blocks * R);
    hipLaunchKernelGGL((k_ln_forward<T, V, L, P, RMS>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
  }));
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, bool RMS>
int backward(const BackwardArgs &a, hipStream_t stream) {
  const int64_t g = gcd(gcd(gcd(a.c, a.xs), a.dys), gcd(a.dstream ? a.dss : 0, a.dx ? a.dxs : 0));
  const int v = piece_width((int)sizeof(T), (int)g, common_alignment({a.x, a.dy, a.dstream, a.dx, a.gamma}), kPieceNorm);
  ME_PIECE_DISPATCH(T, kPieceNorm, v, for_team<V>(a.c / V, [&](auto l, auto p) {
    constexpr int L = decltype(l)::value, P = decltype(p)::value;
    hipLaunchKernelGGL((k_ln_backward<T, V, L, P, RMS>), dim3((unsigned)a.chunks), dim3(kThreads), 0, stream, a);
  }));
  ME_LAUNCH_CHECK();
  return 0;
}

inline int reduce_params(const float *partial, int chunks, int c, float *grad_gamma, float *grad_beta,
                         hipStream_t stream) {
  hipLaunchKernelGGL(k_ln_param_reduce, dim3((unsigned)ceil_div(2 * c, kThreads)), dim3(kThreads), 0, stream, partial,
                     chunks, c, grad_gamma, grad_beta);
  ME_LAUNCH_CHECK();
  return 0;
}

inline unsigned row_grid(int64_t n) {
  const int64_t blocks = ceil_div(n, kThreads / kWave);
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace lnorm
}  // namespace me

using namespace me;
using namespace me::lnorm;

// what the four entry points check alike, before anything else
#define ME_LN_CHECK_SHAPE(n, c)                                      \
  ME_CHECK(c >= 1, "the channel count must be at least 1");          \
  ME_CHECK(n >= 0 && n < (1ll << 31), "the row count must fit in int32")
#define ME_LN_CHECK_WIDTH(c) \
  ME_CHECK(c <= kMaxC, "rows of more than ME_LNORM_MAX_C channels are not served by the fp32 / bf16 kernels")

extern "C" {

int32_t me_lnorm_chunks(int64_t n, int32_t c, int32_t elem_bytes) {
  if (n < 1 || c < 1 || elem_bytes < 1) return 1;
  int64_t g = ceil_div(n * c * elem_bytes, kChunkBytes);
  if (g > kMaxChunks) g = kMaxChunks;
  if (g > n) g = n;
  return (int32_t)g;
}

int64_t me_lnorm_workspace_bytes(int64_t n, int32_t c, int32_t elem_bytes) {
  return (int64_t)me_lnorm_chunks(n, c, elem_bytes) * 2 * (c > 0 ? c : 0) * (int64_t)sizeof(float);
}

int me_lnorm_forward(const void *x_dev, const void *residual_dev, void *stream_out_dev, int32_t is_bf16, int64_t x_stride,
                     int64_t residual_stride, int64_t stream_out_stride, int64_t n, int32_t c, int32_t rms,
                     const float *gamma_dev, const float *beta_dev, float eps, void *y_dev, int64_t y_stride,
                     float *mean_dev, float *rstd_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_LN_CHECK_SHAPE(n, c);
  ME_LN_CHECK_WIDTH(c);
  ME_CHECK(residual_dev == nullptr || stream_out_dev != nullptr, "a residual needs stream_out");
  ME_CHECK(x_stride >= c && y_stride >= c && (residual_dev == nullptr || residual_stride >= c) &&
               (stream_out_dev == nullptr || stream_out_stride >= c),
           "a row stride must be at least c");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && y_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr),
           "x, y, rstd and (for the layer norm) mean must be given");
  ME_CHECK(stream_out_dev == nullptr || residual_dev != nullptr, "stream_out needs a residual");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({x_dev, residual_dev, stream_out_dev, y_dev}, elem) && aligned({gamma_dev, beta_dev}, 4),
           "the operands must be aligned to their element");
  const ForwardArgs a{x_dev, residual_dev, stream_out_dev, y_dev, x_stride, residual_stride, stream_out_stride, y_stride,
                      n, c, 0, gamma_dev, beta_dev, eps, mean_dev, rstd_dev};
  if (is_bf16) return rms ? forward<__bf16, true>(a, stream) : forward<__bf16, false>(a, stream);
  return rms ? forward<float, true>(a, stream) : forward<float, false>(a, stream);
}

int me_lnorm_backward(const void *x_dev, const void *dy_dev, const void *dstream_dev, int32_t is_bf16, int64_t x_stride,
                      int64_t dy_stride, int64_t dstream_stride, int64_t n, int32_t c, int32_t rms,
                      const float *gamma_dev, const float *mean_dev, const float *rstd_dev, void *dx_dev,
                      int64_t dx_stride, float *grad_gamma_dev, float *grad_beta_dev, void *workspace_dev,
                      int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_LN_CHECK_SHAPE(n, c);
  ME_LN_CHECK_WIDTH(c);
  ME_CHECK(x_stride >= c && dy_stride >= c && (dstream_dev == nullptr || dstream_stride >= c) &&
               (dx_dev == nullptr || dx_stride >= c),
           "a row stride must be at least c");
  const bool params = grad_gamma_dev != nullptr || grad_beta_dev != nullptr;
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(!params || (workspace_dev != nullptr && workspace_bytes >= me_lnorm_workspace_bytes(n, c, elem)),
           "a parameter gradient needs a workspace of me_lnorm_workspace_bytes");
  if (n == 0) return params ? reduce_params(nullptr, 0, c, grad_gamma_dev, grad_beta_dev, stream) : 0;
  ME_CHECK(x_dev != nullptr && dy_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr),
           "x, dy, rstd and (for the layer norm) mean must be given");
  ME_CHECK(aligned({x_dev, dy_dev, dstream_dev, dx_dev}, elem) && aligned({gamma_dev, workspace_dev}, 4),
           "the operands must be aligned to their element");
  if (dx_dev == nullptr && !params) return 0;
  const BackwardArgs a{x_dev, dy_dev, dstream_dev, dx_dev, x_stride, dy_stride, dstream_stride, dx_stride, n, c,
                       me_lnorm_chunks(n, c, elem), gamma_dev, mean_dev, rstd_dev,
                       params ? (float *)workspace_dev : nullptr};
  const int rc = is_bf16 ? (rms ? backward<__bf16, true>(a, stream) : backward<__bf16, false>(a, stream))
                         : (rms ? backward<float, true>(a, stream) : backward<float, false>(a, stream));
  if (rc != 0 || !params) return rc;
  return reduce_params(a.partial, a.chunks, c, grad_gamma_dev, grad_beta_dev, stream);
}

int me_lnorm_forward_f64(const double *x_dev, const double *residual_dev, double *stream_out_dev, int64_t x_stride,
                         int64_t residual_stride, int64_t stream_out_stride, int64_t n, int32_t c, int32_t rms,
                         const double *gamma_dev, const double *beta_dev, double eps, double *y_dev, int64_t y_stride,
                         double *mean_dev, double *rstd_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_LN_CHECK_SHAPE(n, c);
  ME_CHECK(residual_dev == nullptr || stream_out_dev != nullptr, "a residual needs stream_out");
  ME_CHECK(x_stride >= c && y_stride >= c && (residual_dev == nullptr || residual_stride >= c) &&
               (stream_out_dev == nullptr || stream_out_stride >= c),
           "a row stride must be at least c");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && y_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr),
           "x, y, rstd and (for the layer norm) mean must be given");
  ME_CHECK(stream_out_dev == nullptr || residual_dev != nullptr, "stream_out needs a residual");
  hipLaunchKernelGGL(k_ln_forward_f64, dim3(row_grid(n)), dim3(kThreads), 0, stream, x_dev, x_stride, residual_dev,
                     residual_stride, stream_out_dev, stream_out_stride, n, (int)c, (int)rms, gamma_dev, beta_dev, eps,
                     y_dev, y_stride, mean_dev, rstd_dev);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_lnorm_backward_f64(const double *x_dev, const double *dy_dev, const double *dstream_dev, int64_t x_stride,
                          int64_t dy_stride, int64_t dstream_stride, int64_t n, int32_t c, int32_t rms,
                          const double *gamma_dev, const double *mean_dev, const double *rstd_dev, double *dx_dev,
                          int64_t dx_stride, double *grad_gamma_dev, double *grad_beta_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_LN_CHECK_SHAPE(n, c);
  ME_CHECK(x_stride >= c && dy_stride >= c && (dstream_dev == nullptr || dstream_stride >= c) &&
               (dx_dev == nullptr || dx_stride >= c),
           "a row stride must be at least c");
  const bool params = grad_gamma_dev != nullptr || grad_beta_dev != nullptr;
  if (n > 0)
    ME_CHECK(x_dev != nullptr && dy_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr),
             "x, dy, rstd and (for the layer norm) mean must be given");
  if (n > 0 && dx_dev != nullptr) {
    hipLaunchKernelGGL(k_ln_backward_f64, dim3(row_grid(n)), dim3(kThreads), 0, stream, x_dev, x_stride, dy_dev,
                       dy_stride, dstream_dev, dstream_stride, n, (int)c, (int)rms, gamma_dev, mean_dev, rstd_dev, dx_dev,
                       dx_stride);
    ME_LAUNCH_CHECK();
  }
  if (params) {
    hipLaunchKernelGGL(k_ln_param_f64, dim3((unsigned)ceil_div(c, kThreads)), dim3(kThreads), 0, stream, x_dev, x_stride,
                       dy_dev, dy_stride, n, (int)c, (int)rms, mean_dev, rstd_dev, grad_gamma_dev, grad_beta_dev);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
