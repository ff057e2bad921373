// Layer norm / RMS norm modulated per instance, with a gated residual add, for gfx950 (MI355X): one half of a DiT block
// (MinkowskiAdaLayerNorm; definition in include/me_amd.h, ABI 1.26)
//
//   stream[r] = T(fma(gate[b], input[r], residual[r]))         b = batch_row[r]; without a residual stream = input
//   normed[r] = T(fma(yhat, 1 + scale[b], shift[b]))           yhat = xhat gamma + beta, xhat as k_ln_forward forms it
//
// One pass forward, one pass plus two small merges backward.  Rows live in the row teams of row_team.hpp, so xhat, the
// stream and dx have the bits layer_norm.hip gives for the same row, and with scale = shift = 0, gate = 1 the whole call
// equals the plain layer bit for bit.
//   * k_adaln_forward is k_ln_forward plus the tables: a team reads b of its row and keeps its pieces of 1 + scale[b],
//     shift[b], gate[b] in registers; they are loaded again only when some team of the wave meets another b (a wave-
//     uniform branch around unguarded loads — rows of a scene are normally consecutive, so this is once per scene and
//     workgroup).  Rows may come in any order; b is clamped into the table.
//   * k_adaln_backward: the chunks are cut over the per-instance row lists, so a workgroup owns a run of rows of ONE
//     instance: instance b of m rows has ceil(m / rc) chunks of rc consecutive list entries, rc = chunk_rows(n, c, e), a
//     pure function of its arguments.  Workgroup g finds (b, first entry) by walking seg_ptr (scalar loads; the
//     surplus workgroups of the grid me_lnorm_chunks + n_batch leave).  Its rows are reached through seg_rows, the next
//     row index fetched a step ahead.  With one instance per workgroup the modulation is a factor of gamma
//     (gm = (1 + scale[b]) gamma, formed once), and the per-lane sums are A = sum dy xhat, B = sum dy and
//     Q = sum input dS over the rows of the chunk — from these
//         dshift[b] = B,  dscale[b] = gamma A + beta B,  dgate[b] = Q,  dgamma += (1 + scale[b]) A,  dbeta += (1 + scale[b]) B
//     so a record is [3][c] whatever is asked for.  Without dy (only the stream was used) the norm terms drop out.
//   * k_adaln_instance_reduce: one thread per (instance, channel) adds the records of the instance in ascending chunk
//     order (8 x 3 loads in flight, the adds in order), writes dshift / dscale / dgate and the instance's [2][c]
//     contribution to dgamma / dbeta; k_adaln_param_reduce adds those in ascending instance order.  No atomics.
//   * The float64 twins are the plain formulas: one wave a row, one thread per (instance, channel) or per channel.
// Byte model: forward (2 + 2 [residual]) n c e, backward (3 + 1 [dstream] + 2 [gate]) n c e; the tables are n_batch c
// floats each and stay in cache.
#include "row_team.hpp"

namespace me {
namespace adaln {
using namespace me::lnorm;

// rows of a chunk of the backward pass: at least kChunkBytes of x, and at most kMaxChunks chunks beside one per instance
__host__ __device__ inline int64_t chunk_rows(int64_t n, int c, int elem) {
  const int64_t a = ((int64_t)kChunkBytes + (int64_t)c * elem - 1) / ((int64_t)c * elem);
  const int64_t b = (n + kMaxChunks - 1) / kMaxChunks;
  return a > b ? a : b;
}

struct ForwardArgs {
  const void *x, *res;
  void *sout, *y;
  int64_t xs, rs, ss, ys, n;
  int c, iters, n_batch;
  const int32_t *batch_row;
  const float *gamma, *beta, *scale, *shift, *gate;
  float eps;
  float *mean, *rstd;
};

template <typename T, int V, int L, int P, bool RMS>
__global__ __launch_bounds__(kThreads) void k_adaln_forward(const ForwardArgs a) {
  constexpr int R = kThreads / L;   // rows of a workgroup per step
  const T *x = (const T *)a.x, *res = (const T *)a.res;
  T *sout = (T *)a.sout, *y = (T *)a.y;
  const int team = threadIdx.x / L;
  const float fc = (float)a.c;
  int ch[P];
  bool ok[P];
  lane_pieces<V, L, P>(a.c, ch, ok);
  float ga[P][V], be[P][V], sc[P][V], sh[P][V], gt[P][V];
  load_param<V, P>(a.gamma, ch, 1.f, ga);
  load_param<V, P>(a.beta, ch, 0.f, be);
  load_param<V, P>(nullptr, ch, 1.f, sc);
  load_param<V, P>(nullptr, ch, 0.f, sh);
  load_param<V, P>(nullptr, ch, 1.f, gt);
  const bool tables = a.scale != nullptr || a.shift != nullptr || a.gate != nullptr;
  int prev = -1;
  for (int it = 0; it < a.iters; ++it) {
    const int64_t row = ((int64_t)it * gridDim.x + blockIdx.x) * R + team;
    const bool live = row < a.n;
    const int64_t r = live ? row : a.n - 1;
    if (tables) {
      int b = a.batch_row[r];
      b = b < 0 ? 0 : b >= a.n_batch ? a.n_batch - 1 : b;
      // some team of the wave changes its instance: every lane loads the pieces of its own b again
      if (__builtin_amdgcn_ballot_w64(b != prev) != 0) {
        const int64_t off = (int64_t)b * a.c;
        load_param<V, P>(a.scale != nullptr ? a.scale + off : nullptr, ch, 0.f, sc);
        load_param<V, P>(a.shift != nullptr ? a.shift + off : nullptr, ch, 0.f, sh);
        load_param<V, P>(a.gate != nullptr ? a.gate + off : nullptr, ch, 1.f, gt);
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int j = 0; j < V; ++j) sc[p][j] = 1.f + sc[p][j];
        prev = b;
      }
    }
    float xv[P][V];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Piece<V> t = load_piece<T, V>(x + r * a.xs + ch[p]);
      if (res != nullptr) {
        const Piece<V> u = load_piece<T, V>(res + r * a.rs + ch[p]);
#pragma unroll
        for (int j = 0; j < V; ++j) t.v[j] = (float)(T)__builtin_fmaf(gt[p][j], t.v[j], u.v[j]);
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
      for (int j = 0; j < V; ++j)
        o.v[j] = __builtin_fmaf(__builtin_fmaf(d[p][j] * rs, ga[p][j], be[p][j]), sc[p][j], sh[p][j]);
      if (live && ok[p]) store_piece<T, V>(y + r * a.ys + ch[p], o);
    }
    if (live && threadIdx.x % L == 0) {
      if constexpr (!RMS) a.mean[row] = mu;
      a.rstd[row] = rs;
    }
  }
}

// chunk g of the rule -> its instance b and its list entries [lo, hi); false for a workgroup past the last chunk
__device__ __forceinline__ bool find_chunk(const int32_t *seg_ptr, int n_batch, int rc, int g, int &b, int &lo, int &hi) {
  for (b = 0; b < n_batch; ++b) {
    const int s = seg_ptr[b], m = seg_ptr[b + 1] - s;
    const int cnt = (m + rc - 1) / rc;
    if (g < cnt) {
      lo = s + g * rc;
      hi = lo + rc < s + m ? lo + rc : s + m;
      return true;
    }
    g -= cnt;
  }
  return false;
}

struct BackwardArgs {
  const void *x, *dy, *dstream, *in;   // x: the rows that were normalised (the stream); dy or dstream may be NULL
  void *dx, *din;                      // dS (the gradient of the stream: of residual, and of input without a gate), gate dS
  int64_t xs, dys, dss, ins, dxs, dis, n;
  int c, n_batch, rc;
  const int32_t *seg_ptr, *seg_rows;
  const float *gamma, *scale, *gate, *rstd;
  float *partial;   // [chunks][3][c]: A, B, Q of a chunk, or NULL
};

template <typename T, int V, int L, int P, bool RMS>
__global__ __launch_bounds__(kThreads) void k_adaln_backward(const BackwardArgs a) {
  constexpr int R = kThreads / L;
  __shared__ float red[kThreads / kWave - 1][L * P * V];
  int b, lo, hi;
  if (!find_chunk(a.seg_ptr, a.n_batch, a.rc, (int)blockIdx.x, b, lo, hi)) return;
  const T *x = (const T *)a.x, *dy = (const T *)a.dy, *dstream = (const T *)a.dstream, *in = (const T *)a.in;
  T *dx = (T *)a.dx, *din = (T *)a.din;
  const int team = threadIdx.x / L;
  const float fc = (float)a.c;
  int ch[P];
  bool ok[P];
  lane_pieces<V, L, P>(a.c, ch, ok);
  // gm = (1 + scale[b]) gamma: the modulation is one factor of the workgroup's instance
  float gm[P][V], gt[P][V], ag[P][V], ab[P][V], aq[P][V];
  load_param<V, P>(a.gamma, ch, 1.f, gm);
  load_param<V, P>(a.scale != nullptr ? a.scale + (int64_t)b * a.c : nullptr, ch, 0.f, gt);
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      gm[p][j] = (1.f + gt[p][j]) * gm[p][j];
      ag[p][j] = ab[p][j] = aq[p][j] = 0.f;
    }
  load_param<V, P>(a.gate != nullptr ? a.gate + (int64_t)b * a.c : nullptr, ch, 1.f, gt);
  const int iters = (hi - lo + R - 1) / R;
  const int64_t top = a.n - 1;
  // the row of list entry e (a dead team reads the chunk's last), clamped into the matrix
  auto row_of = [&](int e) {
    const int64_t r = a.seg_rows[e < hi ? e : hi - 1];
    return r < 0 ? 0 : r > top ? top : r;
  };
  int64_t rnext = row_of(lo + team);
  for (int it = 0; it < iters; ++it) {
    const int e = lo + it * R + team;
    const bool live = e < hi;
    const int64_t r = rnext;
    rnext = row_of(e + R);   // a step ahead: the loads of a row wait for its index
    float xh[P][V], xe[P][V], dyv[P][V], o[P][V];
    if (dy != nullptr) {
      const float rs = a.rstd[r];
      float g[P][V], t1[P][V], t2[P][V];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const Piece<V> xv = load_piece<T, V>(x + r * a.xs + ch[p]);
#pragma unroll
        for (int j = 0; j < V; ++j) t2[p][j] = ok[p] ? xv.v[j] : 0.f;
      }
      // the row is centred again as the forward pass centred it: xhat has the forward's bits
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
          t1[p][j] = g[p][j] = dyv[p][j] * gm[p][j];
          t2[p][j] = g[p][j] * xh[p][j];
        }
      }
      const float m1 = RMS ? 0.f : team_sum<L, P, V>(t1) / fc;
      // s2 with what its products lost to rounding, as k_ln_backward carries it
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < V; ++j) t1[p][j] = __builtin_fmaf(g[p][j], xh[p][j], -t2[p][j]) + g[p][j] * xe[p][j];
      const float s2 = team_sum<L, P, V>(t2), s2lo = team_sum<L, P, V>(t1);
      const float m2 = s2 / fc, m2lo = (__builtin_fmaf(-m2, fc, s2) + s2lo) / fc;
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float t = __builtin_fmaf(-xh[p][j], m2, g[p][j] - m1);
          t = __builtin_fmaf(-xe[p][j], m2, __builtin_fmaf(-xh[p][j], m2lo, t));
          o[p][j] = (float)(T)(t * rs);
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      Piece<V> s;
      if (dstream != nullptr) {
        const Piece<V> u = load_piece<T, V>(dstream + r * a.dss + ch[p]);
#pragma unroll
        for (int j = 0; j < V; ++j) s.v[j] = dy != nullptr ? (float)(T)(o[p][j] + u.v[j]) : u.v[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) s.v[j] = o[p][j];
      }
      if (dx != nullptr && live && ok[p]) store_piece<T, V>(dx + r * a.dxs + ch[p], s);
      if (in != nullptr) {
        const Piece<V> u = load_piece<T, V>(in + r * a.ins + ch[p]);
        Piece<V> q;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          q.v[j] = gt[p][j] * s.v[j];
          aq[p][j] = live && ok[p] ? __builtin_fmaf(u.v[j], s.v[j], aq[p][j]) : aq[p][j];
        }
        if (din != nullptr && live && ok[p]) store_piece<T, V>(din + r * a.dis + ch[p], q);
      }
      if (dy != nullptr) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          ag[p][j] = live ? __builtin_fmaf(dyv[p][j], xh[p][j], __builtin_fmaf(dyv[p][j], xe[p][j], ag[p][j])) : ag[p][j];
          ab[p][j] = live ? ab[p][j] + dyv[p][j] : ab[p][j];
        }
      }
    }
  }
  if (a.partial == nullptr) return;
  // the teams of a wave, then the waves in wave order, one sum after the other through one buffer
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float *rec = a.partial + (int64_t)blockIdx.x * 3 * a.c;
#pragma unroll
  for (int which = 0; which < 3; ++which) {
    if (which == 2 && in == nullptr) break;
    float(&acc)[P][V] = which == 0 ? ag : which == 1 ? ab : aq;
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

// the records of instance blockIdx.y in ascending chunk order, per channel -> dshift, dscale, dgate of the instance and
// its contribution inst[b][2][c] to dgamma / dbeta (each written only where asked for); an instance without rows gives 0
__global__ __launch_bounds__(kThreads) void k_adaln_instance_reduce(
    const float *__restrict__ partial, const int32_t *__restrict__ seg_ptr, int rc, int c, int has_q,
    const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ scale,
    float *__restrict__ grad_scale, float *__restrict__ grad_shift, float *__restrict__ grad_gate,
    float *__restrict__ inst) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (ch >= c) return;
  int first = 0;
  for (int i = 0; i < b; ++i) first += (seg_ptr[i + 1] - seg_ptr[i] + rc - 1) / rc;
  const int cnt = (seg_ptr[b + 1] - seg_ptr[b] + rc - 1) / rc;
  const float *rec = partial + (int64_t)first * 3 * c + ch;
  float sa = 0.f, sb = 0.f, sq = 0.f;
  // (the adds stay in ascending chunk order; unrolled so that the loads of 8 chunks are in flight)
  if (has_q) {
#pragma unroll 8
    for (int g = 0; g < cnt; ++g) {
      sa += rec[((int64_t)g * 3 + 0) * c];
      sb += rec[((int64_t)g * 3 + 1) * c];
      sq += rec[((int64_t)g * 3 + 2) * c];
    }
  } else {
#pragma unroll 8
    for (int g = 0; g < cnt; ++g) {
      sa += rec[((int64_t)g * 3 + 0) * c];
      sb += rec[((int64_t)g * 3 + 1) * c];
    }
  }
  const int64_t o = (int64_t)b * c + ch;
  if (grad_shift != nullptr) grad_shift[o] = sb;
  if (grad_scale != nullptr)
    grad_scale[o] = __builtin_fmaf(gamma != nullptr ? gamma[ch] : 1.f, sa, (beta != nullptr ? beta[ch] : 0.f) * sb);
  if (grad_gate != nullptr) grad_gate[o] = sq;
  if (inst != nullptr) {
    const float s1 = 1.f + (scale != nullptr ? scale[o] : 0.f);
    inst[((int64_t)b * 2 + 0) * c + ch] = s1 * sa;
    inst[((int64_t)b * 2 + 1) * c + ch] = s1 * sb;
  }
}

// grad_gamma[ch] / grad_beta[ch] = the contributions of the instances in ascending order; n_batch = 0 writes zeros
__global__ __launch_bounds__(kThreads) void k_adaln_param_reduce(const float *__restrict__ inst, int n_batch, int c,
                                                                 float *__restrict__ grad_gamma,
                                                                 float *__restrict__ grad_beta) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * c) return;
  const int which = idx / c, ch = idx - which * c;
  float *dst = which == 0 ? grad_gamma : grad_beta;
  if (dst == nullptr) return;
  float s = 0.f;
#pragma unroll 16
  for (int b = 0; b < n_batch; ++b) s += inst[((int64_t)b * 2 + which) * c + ch];
  dst[ch] = s;
}

// ---- float64 twins: the plain formulas ------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct ArgsF64 {
  const double *x, *res, *dy, *dstream, *in;   // forward: x = input; backward: x = the stream
  double *sout, *y, *dx, *din;
  int64_t xs, rs, ss, ys, dys, dss, ins, dxs, dis, n;
  int c, rms, n_batch;
  const int32_t *batch_row, *seg_ptr, *seg_rows;
  const double *gamma, *beta, *scale, *shift, *gate;
  double eps;
  double *mean, *rstd, *grad_gamma, *grad_beta, *grad_scale, *grad_shift, *grad_gate;
};

__device__ __forceinline__ int clamp_b(int b, int n_batch) { return b < 0 ? 0 : b >= n_batch ? n_batch - 1 : b; }

// one wave a row, the lanes stride over the channels
__global__ __launch_bounds__(kThreads) void k_adaln_forward_f64(const ArgsF64 a) {
  const int lane = lane_id();
  const int64_t step = (int64_t)gridDim.x * (kThreads / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; r < a.n; r += step) {
    const int64_t t = (int64_t)clamp_b(a.batch_row[r], a.n_batch) * a.c;
    auto s_of = [&](int ch) {
      const double v = a.x[r * a.xs + ch];
      return a.res != nullptr ? fma(a.gate != nullptr ? a.gate[t + ch] : 1.0, v, a.res[r * a.rs + ch]) : v;
    };
    double s = 0.0;
    for (int ch = lane; ch < a.c; ch += kWave) {
      const double v = s_of(ch);
      if (a.res != nullptr) a.sout[r * a.ss + ch] = v;
      s += v;
    }
    const double mu = a.rms ? 0.0 : wave_sum(s) / a.c;
    double q = 0.0;
    for (int ch = lane; ch < a.c; ch += kWave) {
      const double v = s_of(ch) - mu;
      q += v * v;
    }
    const double rd = 1.0 / sqrt(wave_sum(q) / a.c + a.eps);
    for (int ch = lane; ch < a.c; ch += kWave) {
      const double yh = (s_of(ch) - mu) * rd * (a.gamma != nullptr ? a.gamma[ch] : 1.0) +
                        (a.beta != nullptr ? a.beta[ch] : 0.0);
      a.y[r * a.ys + ch] = yh * (1.0 + (a.scale != nullptr ? a.scale[t + ch] : 0.0)) +
                           (a.shift != nullptr ? a.shift[t + ch] : 0.0);
    }
    if (lane == 0) {
      if (!a.rms) a.mean[r] = mu;
      a.rstd[r] = rd;
    }
  }
}

// dS of row r and channel ch from the row sums s1 / c, s2 / c (0 when dy is absent)
__device__ __forceinline__ double ds_f64(const ArgsF64 &a, int64_t r, int64_t t, int ch, double mu, double rd, double s1,
                                         double s2) {
  double v = a.dstream != nullptr ? a.dstream[r * a.dss + ch] : 0.0;
  if (a.dy != nullptr) {
    const double g = a.dy[r * a.dys + ch] * (1.0 + (a.scale != nullptr ? a.scale[t + ch] : 0.0)) *
                     (a.gamma != nullptr ? a.gamma[ch] : 1.0);
    v += (g - (s1 + (a.x[r * a.xs + ch] - mu) * rd * s2)) * rd;
  }
  return v;
}

// the two row sums of the layer-norm gradient, by the calling wave
__device__ __forceinline__ void row_sums_f64(const ArgsF64 &a, int64_t r, int64_t t, int lane, double mu, double rd,
                                             double &s1, double &s2) {
  s1 = s2 = 0.0;
  if (a.dy == nullptr) return;
  for (int ch = lane; ch < a.c; ch += kWave) {
    const double g = a.dy[r * a.dys + ch] * (1.0 + (a.scale != nullptr ? a.scale[t + ch] : 0.0)) *
                     (a.gamma != nullptr ? a.gamma[ch] : 1.0);
    s1 += g;
    s2 += g * ((a.x[r * a.xs + ch] - mu) * rd);
  }
  s1 = a.rms ? 0.0 : wave_sum(s1) / a.c;
  s2 = wave_sum(s2) / a.c;
}

__global__ __launch_bounds__(kThreads) void k_adaln_backward_f64(const ArgsF64 a) {
  const int lane = lane_id();
  const int64_t step = (int64_t)gridDim.x * (kThreads / kWave);
  for (int64_t r = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; r < a.n; r += step) {
    const int64_t t = (int64_t)clamp_b(a.batch_row[r], a.n_batch) * a.c;
    const double mu = a.rms || a.dy == nullptr ? 0.0 : a.mean[r], rd = a.dy == nullptr ? 0.0 : a.rstd[r];
    double s1, s2;
    row_sums_f64(a, r, t, lane, mu, rd, s1, s2);
    for (int ch = lane; ch < a.c; ch += kWave) {
      const double v = ds_f64(a, r, t, ch, mu, rd, s1, s2);
      if (a.dx != nullptr) a.dx[r * a.dxs + ch] = v;
      if (a.din != nullptr) a.din[r * a.dis + ch] = (a.gate != nullptr ? a.gate[t + ch] : 1.0) * v;
    }
  }
}

// dgate: one wave per row would need the row sums again per channel, so a wave takes an instance's rows in ascending
// order and its lanes stride over the channels (blockIdx.x = instance, one wave)
__global__ __launch_bounds__(kWave) void k_adaln_gate_f64(const ArgsF64 a) {
  const int lane = lane_id(), b = blockIdx.x;
  const int64_t t = (int64_t)b * a.c;
  for (int c0 = 0; c0 < a.c; c0 += kWave) {
    const int ch = c0 + lane;
    double q = 0.0;
    for (int e = a.seg_ptr[b]; e < a.seg_ptr[b + 1]; ++e) {
      int64_t r = a.seg_rows[e];
      r = r < 0 ? 0 : r >= a.n ? a.n - 1 : r;
      const double mu = a.rms || a.dy == nullptr ? 0.0 : a.mean[r], rd = a.dy == nullptr ? 0.0 : a.rstd[r];
      double s1, s2;
      row_sums_f64(a, r, t, lane, mu, rd, s1, s2);
      if (ch < a.c) q += a.in[r * a.ins + ch] * ds_f64(a, r, t, ch, mu, rd, s1, s2);
    }
    if (ch < a.c) a.grad_gate[t + ch] = q;
  }
}

// dscale / dshift: one thread per (instance, channel), the rows of the instance in ascending order
__global__ __launch_bounds__(kThreads) void k_adaln_mod_f64(const ArgsF64 a) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (ch >= a.c) return;
  double ss = 0.0, sh = 0.0;
  for (int e = a.seg_ptr[b]; e < a.seg_ptr[b + 1]; ++e) {
    int64_t r = a.seg_rows[e];
    r = r < 0 ? 0 : r >= a.n ? a.n - 1 : r;
    const double d = a.dy[r * a.dys + ch];
    const double xh = (a.x[r * a.xs + ch] - (a.rms ? 0.0 : a.mean[r])) * a.rstd[r];
    ss += d * (xh * (a.gamma != nullptr ? a.gamma[ch] : 1.0) + (a.beta != nullptr ? a.beta[ch] : 0.0));
    sh += d;
  }
  if (a.grad_scale != nullptr) a.grad_scale[(int64_t)b * a.c + ch] = ss;
  if (a.grad_shift != nullptr) a.grad_shift[(int64_t)b * a.c + ch] = sh;
}

// dgamma / dbeta: one thread a channel, the rows in ascending order
__global__ __launch_bounds__(kThreads) void k_adaln_param_f64(const ArgsF64 a) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= a.c) return;
  double sg = 0.0, sb = 0.0;
  for (int64_t r = 0; r < a.n; ++r) {
    const int64_t t = (int64_t)clamp_b(a.batch_row[r], a.n_batch) * a.c;
    const double d = a.dy[r * a.dys + ch] * (1.0 + (a.scale != nullptr ? a.scale[t + ch] : 0.0));
    sg += d * ((a.x[r * a.xs + ch] - (a.rms ? 0.0 : a.mean[r])) * a.rstd[r]);
    sb += d;
  }
  if (a.grad_gamma != nullptr) a.grad_gamma[ch] = sg;
  if (a.grad_beta != nullptr) a.grad_beta[ch] = sb;
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <typename T, bool RMS>
int forward(ForwardArgs a, hipStream_t stream) {
  const int64_t g = gcd(gcd(gcd(a.c, a.xs), a.ys), gcd(a.res ? a.rs : 0, a.sout ? a.ss : 0));
  const int v = piece_width((int)sizeof(T), (int)g,
                            common_alignment({a.x, a.res, a.sout, a.y, a.gamma, a.beta, a.scale, a.shift, a.gate}),
                            kPieceNorm);
  ME_PIECE_DISPATCH(T, kPieceNorm, v, for_team<V>(a.c / V, [&](auto l, auto p) {
    constexpr int L = decltype(l)::value, P = decltype(p)::value, R = kThreads / L;
    const int64_t blocks = ceil_div(a.n, R) < kMaxBlocks ? ceil_div(a.n, R) : kMaxBlocks;
    a.iters = (int)ceil_div(a.n, blocks * R);
    hipLaunchKernelGGL((k_adaln_forward<T, V, L, P, RMS>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
  }));
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, bool RMS>
int backward(const BackwardArgs &a, unsigned grid, hipStream_t stream) {
  const int64_t g = gcd(gcd(gcd(a.c, a.xs), gcd(a.dy ? a.dys : 0, a.dstream ? a.dss : 0)),
                        gcd(gcd(a.dx ? a.dxs : 0, a.in ? a.ins : 0), a.din ? a.dis : 0));
  const int v = piece_width((int)sizeof(T), (int)g,
                            common_alignment({a.x, a.dy, a.dstream, a.in, a.dx, a.din, a.gamma, a.scale, a.gate}),
                            kPieceNorm);
  ME_PIECE_DISPATCH(T, kPieceNorm, v, for_team<V>(a.c / V, [&](auto l, auto p) {
    constexpr int L = decltype(l)::value, P = decltype(p)::value;
    hipLaunchKernelGGL((k_adaln_backward<T, V, L, P, RMS>), dim3(grid), dim3(kThreads), 0, stream, a);
  }));
  ME_LAUNCH_CHECK();
  return 0;
}

inline unsigned row_grid(int64_t n) {
  const int64_t blocks = ceil_div(n, kThreads / kWave);
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace adaln
}  // namespace me

using namespace me;
using namespace me::adaln;

// what the entry points check alike, before anything else
#define ME_ADALN_CHECK_SHAPE(n, c, n_batch)                                    \
  ME_CHECK(c >= 1, "the channel count must be at least 1");                    \
  ME_CHECK(n >= 0 && n < (1ll << 31), "the row count must fit in int32");      \
  ME_CHECK(n_batch >= 0 && (n == 0 || n_batch >= 1), "rows need at least one instance")
#define ME_ADALN_CHECK_WIDTH(c) \
  ME_CHECK(c <= kMaxC, "rows of more than ME_LNORM_MAX_C channels are not served by the fp32 / bf16 kernels")

extern "C" {

int32_t me_adaln_chunks(int64_t n, int32_t n_batch, int32_t c, int32_t elem_bytes) {
  return me_lnorm_chunks(n, c, elem_bytes) + (n_batch > 0 ? n_batch : 0);
}

int64_t me_adaln_workspace_bytes(int64_t n, int32_t n_batch, int32_t c, int32_t elem_bytes) {
  const int64_t cc = c > 0 ? c : 0, nb = n_batch > 0 ? n_batch : 0;
  return ((int64_t)me_adaln_chunks(n, n_batch, c, elem_bytes) * 3 + nb * 2) * cc * (int64_t)sizeof(float);
}

int me_adaln_forward(const void *x_dev, const void *residual_dev, void *stream_out_dev, int32_t is_bf16, int64_t x_stride,
                     int64_t residual_stride, int64_t stream_out_stride, int64_t n, int32_t c, int32_t rms,
                     const int32_t *batch_row_dev, int32_t n_batch, const float *gamma_dev, const float *beta_dev,
                     const float *scale_dev, const float *shift_dev, const float *gate_dev, float eps, void *y_dev,
                     int64_t y_stride, float *mean_dev, float *rstd_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_ADALN_CHECK_SHAPE(n, c, n_batch);
  ME_ADALN_CHECK_WIDTH(c);
  ME_CHECK(residual_dev == nullptr || stream_out_dev != nullptr, "a residual needs stream_out");
  ME_CHECK(gate_dev == nullptr || residual_dev != nullptr, "a gate needs a residual");
  ME_CHECK(x_stride >= c && y_stride >= c && (residual_dev == nullptr || residual_stride >= c) &&
               (stream_out_dev == nullptr || stream_out_stride >= c),
           "a row stride must be at least c");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && y_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr),
           "x, y, rstd and (for the layer norm) mean must be given");
  ME_CHECK(stream_out_dev == nullptr || residual_dev != nullptr, "stream_out needs a residual");
  const bool tables = scale_dev != nullptr || shift_dev != nullptr || gate_dev != nullptr;
  ME_CHECK(!tables || batch_row_dev != nullptr, "scale, shift and gate need batch_row");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({x_dev, residual_dev, stream_out_dev, y_dev}, elem) &&
               aligned({gamma_dev, beta_dev, scale_dev, shift_dev, gate_dev, batch_row_dev}, 4),
           "the operands must be aligned to their element");
  const adaln::ForwardArgs a{x_dev, residual_dev, stream_out_dev, y_dev, x_stride, residual_stride, stream_out_stride,
                             y_stride, n, c, 0, n_batch, batch_row_dev, gamma_dev, beta_dev, scale_dev, shift_dev,
                             gate_dev, eps, mean_dev, rstd_dev};
  if (is_bf16) return rms ? adaln::forward<__bf16, true>(a, stream) : adaln::forward<__bf16, false>(a, stream);
  return rms ? adaln::forward<float, true>(a, stream) : adaln::forward<float, false>(a, stream);
}

int me_adaln_backward(const void *stream_rows_dev, const void *dy_dev, const void *dstream_dev, const void *input_dev,
                      int32_t is_bf16, int64_t x_stride, int64_t dy_stride, int64_t dstream_stride, int64_t input_stride,
                      int64_t n, int32_t c, int32_t rms, const int32_t *seg_ptr_dev, const int32_t *seg_rows_dev,
                      int32_t n_batch, const float *gamma_dev, const float *beta_dev, const float *scale_dev,
                      const float *gate_dev, const float *rstd_dev, void *dstream_out_dev, int64_t dstream_out_stride,
                      void *dinput_dev, int64_t dinput_stride, float *grad_gamma_dev, float *grad_beta_dev,
                      float *grad_scale_dev, float *grad_shift_dev, float *grad_gate_dev, void *workspace_dev,
                      int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_ADALN_CHECK_SHAPE(n, c, n_batch);
  ME_ADALN_CHECK_WIDTH(c);
  ME_CHECK((dy_dev == nullptr || (x_stride >= c && dy_stride >= c)) && (dstream_dev == nullptr || dstream_stride >= c) &&
               (input_dev == nullptr || input_stride >= c) && (dstream_out_dev == nullptr || dstream_out_stride >= c) &&
               (dinput_dev == nullptr || dinput_stride >= c),
           "a row stride must be at least c");
  ME_CHECK((gate_dev == nullptr) == (input_dev == nullptr), "gate and input are given together");
  ME_CHECK(dinput_dev == nullptr || gate_dev != nullptr, "dinput needs a gate (without one it is dstream_out)");
  ME_CHECK(grad_gate_dev == nullptr || gate_dev != nullptr, "grad_gate needs a gate");
  ME_CHECK(dy_dev != nullptr || (grad_gamma_dev == nullptr && grad_beta_dev == nullptr && grad_scale_dev == nullptr &&
                                 grad_shift_dev == nullptr),
           "the gradients of gamma, beta, scale and shift need dy");
  const bool mods = grad_scale_dev != nullptr || grad_shift_dev != nullptr || grad_gate_dev != nullptr;
  const bool params = grad_gamma_dev != nullptr || grad_beta_dev != nullptr;
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(!(mods || params) ||
               (workspace_dev != nullptr && workspace_bytes >= me_adaln_workspace_bytes(n, n_batch, c, elem)),
           "a parameter or modulation gradient needs a workspace of me_adaln_workspace_bytes");
  const int grid = me_adaln_chunks(n, n_batch, c, elem);
  const int rc = (int)chunk_rows(n, c, elem);
  float *partial = (float *)workspace_dev, *inst = partial + (int64_t)grid * 3 * c;
  if (n > 0) {
    ME_CHECK(dy_dev != nullptr || dstream_dev != nullptr, "dy or dstream must be given");
    ME_CHECK(seg_ptr_dev != nullptr && seg_rows_dev != nullptr, "the per-instance row lists must be given");
    ME_CHECK(dy_dev == nullptr || (stream_rows_dev != nullptr && rstd_dev != nullptr),
             "the normalised rows and rstd must be given with dy");
    ME_CHECK(aligned({stream_rows_dev, dy_dev, dstream_dev, input_dev, dstream_out_dev, dinput_dev}, elem) &&
                 aligned({gamma_dev, beta_dev, scale_dev, gate_dev, workspace_dev, seg_ptr_dev, seg_rows_dev}, 4),
             "the operands must be aligned to their element");
    if (dstream_out_dev != nullptr || dinput_dev != nullptr || mods || params) {
      const adaln::BackwardArgs a{stream_rows_dev, dy_dev, dstream_dev, input_dev, dstream_out_dev, dinput_dev, x_stride,
                                  dy_stride, dstream_stride, input_stride, dstream_out_stride, dinput_stride, n, c,
                                  n_batch, rc, seg_ptr_dev, seg_rows_dev, gamma_dev, scale_dev, gate_dev, rstd_dev,
                                  mods || params ? partial : nullptr};
      const int rcode = is_bf16 ? (rms ? adaln::backward<__bf16, true>(a, grid, stream)
                                       : adaln::backward<__bf16, false>(a, grid, stream))
                                : (rms ? adaln::backward<float, true>(a, grid, stream)
                                       : adaln::backward<float, false>(a, grid, stream));
      if (rcode != 0) return rcode;
    }
  } else if (n_batch > 0 && (mods || params)) {
    ME_CHECK(seg_ptr_dev != nullptr, "the per-instance row lists must be given");
  }
  if ((mods || params) && n_batch > 0) {
    hipLaunchKernelGGL(k_adaln_instance_reduce, dim3((unsigned)ceil_div(c, kThreads), (unsigned)n_batch), dim3(kThreads),
                       0, stream, partial, seg_ptr_dev, rc, (int)c, gate_dev != nullptr ? 1 : 0, gamma_dev, beta_dev,
                       scale_dev, grad_scale_dev, grad_shift_dev, grad_gate_dev, params ? inst : nullptr);
    ME_LAUNCH_CHECK();
  }
  if (params) {
    hipLaunchKernelGGL(k_adaln_param_reduce, dim3((unsigned)ceil_div(2 * c, kThreads)), dim3(kThreads), 0, stream, inst,
                       (int)n_batch, (int)c, grad_gamma_dev, grad_beta_dev);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

int me_adaln_forward_f64(const double *x_dev, const double *residual_dev, double *stream_out_dev, int64_t x_stride,
                         int64_t residual_stride, int64_t stream_out_stride, int64_t n, int32_t c, int32_t rms,
                         const int32_t *batch_row_dev, int32_t n_batch, const double *gamma_dev, const double *beta_dev,
                         const double *scale_dev, const double *shift_dev, const double *gate_dev, double eps,
                         double *y_dev, int64_t y_stride, double *mean_dev, double *rstd_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_ADALN_CHECK_SHAPE(n, c, n_batch);
  ME_CHECK(residual_dev == nullptr || stream_out_dev != nullptr, "a residual needs stream_out");
  ME_CHECK(gate_dev == nullptr || residual_dev != nullptr, "a gate needs a residual");
  ME_CHECK(x_stride >= c && y_stride >= c && (residual_dev == nullptr || residual_stride >= c) &&
               (stream_out_dev == nullptr || stream_out_stride >= c),
           "a row stride must be at least c");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && y_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr) &&
               batch_row_dev != nullptr,
           "x, y, rstd, batch_row and (for the layer norm) mean must be given");
  ME_CHECK(stream_out_dev == nullptr || residual_dev != nullptr, "stream_out needs a residual");
  ArgsF64 a{};
  a.x = x_dev, a.res = residual_dev, a.sout = stream_out_dev, a.y = y_dev;
  a.xs = x_stride, a.rs = residual_stride, a.ss = stream_out_stride, a.ys = y_stride, a.n = n;
  a.c = c, a.rms = rms, a.n_batch = n_batch, a.batch_row = batch_row_dev;
  a.gamma = gamma_dev, a.beta = beta_dev, a.scale = scale_dev, a.shift = shift_dev, a.gate = gate_dev;
  a.eps = eps, a.mean = mean_dev, a.rstd = rstd_dev;
  hipLaunchKernelGGL(k_adaln_forward_f64, dim3(row_grid(n)), dim3(kThreads), 0, stream, a);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_adaln_backward_f64(const double *stream_rows_dev, const double *dy_dev, const double *dstream_dev,
                          const double *input_dev, int64_t x_stride, int64_t dy_stride, int64_t dstream_stride,
                          int64_t input_stride, int64_t n, int32_t c, int32_t rms, const int32_t *batch_row_dev,
                          const int32_t *seg_ptr_dev, const int32_t *seg_rows_dev, int32_t n_batch,
                          const double *gamma_dev, const double *beta_dev, const double *scale_dev,
                          const double *gate_dev, const double *mean_dev, const double *rstd_dev,
                          double *dstream_out_dev, int64_t dstream_out_stride, double *dinput_dev, int64_t dinput_stride,
                          double *grad_gamma_dev, double *grad_beta_dev, double *grad_scale_dev, double *grad_shift_dev,
                          double *grad_gate_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_ADALN_CHECK_SHAPE(n, c, n_batch);
  ME_CHECK((dy_dev == nullptr || (x_stride >= c && dy_stride >= c)) && (dstream_dev == nullptr || dstream_stride >= c) &&
               (input_dev == nullptr || input_stride >= c) && (dstream_out_dev == nullptr || dstream_out_stride >= c) &&
               (dinput_dev == nullptr || dinput_stride >= c),
           "a row stride must be at least c");
  ME_CHECK((gate_dev == nullptr) == (input_dev == nullptr), "gate and input are given together");
  ME_CHECK(dinput_dev == nullptr || gate_dev != nullptr, "dinput needs a gate (without one it is dstream_out)");
  ME_CHECK(grad_gate_dev == nullptr || gate_dev != nullptr, "grad_gate needs a gate");
  ME_CHECK(dy_dev != nullptr || (grad_gamma_dev == nullptr && grad_beta_dev == nullptr && grad_scale_dev == nullptr &&
                                 grad_shift_dev == nullptr),
           "the gradients of gamma, beta, scale and shift need dy");
  const bool mods = grad_scale_dev != nullptr || grad_shift_dev != nullptr;
  const bool params = grad_gamma_dev != nullptr || grad_beta_dev != nullptr;
  if (n > 0) {
    ME_CHECK(dy_dev != nullptr || dstream_dev != nullptr, "dy or dstream must be given");
    ME_CHECK(batch_row_dev != nullptr && seg_ptr_dev != nullptr && seg_rows_dev != nullptr,
             "batch_row and the per-instance row lists must be given");
    ME_CHECK(dy_dev == nullptr || (stream_rows_dev != nullptr && rstd_dev != nullptr && (rms || mean_dev != nullptr)),
             "the normalised rows, rstd and (for the layer norm) mean must be given with dy");
  } else if (n_batch > 0 && (mods || grad_gate_dev != nullptr)) {
    ME_CHECK(seg_ptr_dev != nullptr, "the per-instance row lists must be given");
  }
  ArgsF64 a{};
  a.x = stream_rows_dev, a.dy = dy_dev, a.dstream = dstream_dev, a.in = input_dev;
  a.dx = dstream_out_dev, a.din = dinput_dev;
  a.xs = x_stride, a.dys = dy_stride, a.dss = dstream_stride, a.ins = input_stride;
  a.dxs = dstream_out_stride, a.dis = dinput_stride, a.n = n;
  a.c = c, a.rms = rms, a.n_batch = n_batch;
  a.batch_row = batch_row_dev, a.seg_ptr = seg_ptr_dev, a.seg_rows = seg_rows_dev;
  a.gamma = gamma_dev, a.beta = beta_dev, a.scale = scale_dev, a.gate = gate_dev;
  a.mean = (double *)mean_dev, a.rstd = (double *)rstd_dev;
  a.grad_gamma = grad_gamma_dev, a.grad_beta = grad_beta_dev, a.grad_scale = grad_scale_dev;
  a.grad_shift = grad_shift_dev, a.grad_gate = grad_gate_dev;
  if (n > 0 && (dstream_out_dev != nullptr || dinput_dev != nullptr)) {
    hipLaunchKernelGGL(k_adaln_backward_f64, dim3(row_grid(n)), dim3(kThreads), 0, stream, a);
    ME_LAUNCH_CHECK();
  }
  if (grad_gate_dev != nullptr && n_batch > 0) {
    hipLaunchKernelGGL(k_adaln_gate_f64, dim3((unsigned)n_batch), dim3(kWave), 0, stream, a);
    ME_LAUNCH_CHECK();
  }
  if (mods && n_batch > 0) {
    hipLaunchKernelGGL(k_adaln_mod_f64, dim3((unsigned)ceil_div(c, kThreads), (unsigned)n_batch), dim3(kThreads), 0,
                       stream, a);
    ME_LAUNCH_CHECK();
  }
  if (params) {
    hipLaunchKernelGGL(k_adaln_param_f64, dim3((unsigned)ceil_div(c, kThreads)), dim3(kThreads), 0, stream, a);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
