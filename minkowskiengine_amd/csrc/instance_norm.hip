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
//   forward     k_in_apply        y = (x - mean[b]) * rstd[b] * gamma + beta; the coefficients of an instance stay in
//                                 registers while consecutive rows of the thread share the batch index
//   backward    k_in_bwd_partial / k_in_bwd_final   t1[b] = sum dy, t2[b] = sum dy * xhat per (instance, channel)
//               k_in_bwd_params   grad_beta = sum_b t1[b], grad_gamma = sum_b t2[b] (ascending b)
//               k_in_bwd_apply    dx = gamma * rstd[b] * (dy - t1[b] / n_b - xhat * t2[b] / n_b)
// No atomics on values, every sum in a fixed order: bitwise reproducible.  T = float or __bf16 rows; statistics and
// parameters fp32.  The float64 twins at the end are the gradcheck yardstick (plain double, one thread per output).
#include "norm_common.hpp"

#include <limits.h>

namespace me {

// LDS of the partial kernels: bn_partial_lds_bytes.  The 4 ints of the range and per-instance scans of a chunk live in
// s_tmp: bn_reduce_lanes alone writes s_tmp, after its leading barrier (every scan result has been read by then), and has
// read it for the last time before its trailing barrier (the next scan starts after that).  5 c + 256 floats with one row
// lane: rows of up to 3225 channels fit into 64 KiB.
__host__ __device__ constexpr size_t in_partial_lds_bytes(int c, int row_lanes) {
  return bn_partial_lds_bytes(c, row_lanes);
}

template <int V>
__device__ __forceinline__ void load_f32(const float *__restrict__ p, float (&v)[V]) {
  if constexpr (V % 4 == 0) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4 *>(p + 4 * q);
      v[4 * q + 0] = t.x;
      v[4 * q + 1] = t.y;
      v[4 * q + 2] = t.z;
      v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = p[j];
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// smallest and largest batch index among rows [r0, r1), clamped to [0, n_batch) (an index outside it matches no instance
// and is never used as an address).  s_i: 2 ints of LDS.  Integer min / max: the order of the LDS atomics does not matter.
__device__ __forceinline__ void in_scan_range(const int32_t *__restrict__ batch_row, int64_t r0, int64_t r1, int n_batch,
                                              int *s_i, int &bmin, int &bmax) {
  if (threadIdx.x == 0) {
    s_i[0] = INT_MAX;
    s_i[1] = -1;
  }
  __syncthreads();
  int lo = INT_MAX, hi = -1;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    const int b = batch_row[r];
    lo = min(lo, b);
    hi = max(hi, b);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&s_i[0], lo);
    atomicMax(&s_i[1], hi);
  }
  __syncthreads();
  bmin = max(s_i[0], 0);
  bmax = min(s_i[1], n_batch - 1);
}

// first row (relative to r0) and number of rows of batch index b among rows [r0, r1).  s_i: 2 ints of LDS; the caller
// synchronises before it calls this again.
__device__ __forceinline__ void in_scan_instance(const int32_t *__restrict__ batch_row, int64_t r0, int64_t r1, int b,
                                                 int *s_i, int &first, int &count) {
  if (threadIdx.x == 0) {
    s_i[0] = INT_MAX;
    s_i[1] = 0;
  }
  __syncthreads();
  int f = INT_MAX, k = 0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    if (batch_row[r] == b) {
      f = min(f, (int)(r - r0));
      ++k;
    }
  }
  f = wave_min(f);
  k = wave_sum(k);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&s_i[0], f);
    atomicAdd(&s_i[1], k);
  }
  __syncthreads();
  first = s_i[0];
  count = s_i[1];
}

// Per (chunk g, instance b, channel): count, mean and M2 = sum (x - mean)^2 of the rows of b in the chunk, from sums
// shifted by the first such row.  part_mean / part_m2: [chunks][n_batch][c]; part_cnt: [chunks][n_batch], ZEROED by the
// host — only the (g, b) with rows are written, and only those are read by k_in_final.
// Thread layout and load-first structure of k_bn_partial (norm.hip): P = c / V pieces per row, R row lanes, every load of a
// batch of rows unconditional (row clamped to the chunk) with the contribution selected afterwards.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_in_partial(const T *__restrict__ x, const int32_t *__restrict__ batch_row,
                                                   int64_t n, int c, int chunks, int n_batch,
                                                   float *__restrict__ part_mean, float *__restrict__ part_m2,
                                                   float *__restrict__ part_cnt) {
  extern __shared__ float s_red[];  // in_partial_lds_bytes
  const int P = c / V;
  const int W = min(P, (int)blockDim.x);
  const int R = max(1, (int)blockDim.x / P);
  float *s_out = s_red + (size_t)R * 2 * c, *s_tmp = s_out + 2 * c, *s_shift = s_tmp + 256;
  int *s_i = reinterpret_cast<int *>(s_tmp);
  const int64_t r0 = chunk_begin(blockIdx.x, n, chunks), r1 = chunk_begin(blockIdx.x + 1, n, chunks);
  if (r0 >= r1) return;  // whole workgroup
  int bmin, bmax;
  in_scan_range(batch_row, r0, r1, n_batch, s_i, bmin, bmax);
  const bool pure = bmin == bmax;
  for (int b = bmin; b <= bmax; ++b) {   // (uniform: every thread sees the same range)
    int first = 0, count = (int)(r1 - r0);
    if (!pure) {
      in_scan_instance(batch_row, r0, r1, b, s_i + 2, first, count);
      if (count == 0) {   // uniform
        __syncthreads();
        continue;
      }
    }
    for (int p0 = 0; p0 < P; p0 += blockDim.x) {  // one pass unless c / V > blockDim
      const int p = p0 + (int)threadIdx.x % W;
      const int rl = (int)threadIdx.x / W;
      const bool active = rl < R && p < P;
      float s1[V], s2[V], shift[V];
#pragma unroll
      for (int j = 0; j < V; ++j) s1[j] = s2[j] = shift[j] = 0.f;
      if (active) {
        const T *xp = x + p * V;
        const Row<T, V> k = load_row<T, V>(xp + (r0 + first) * c);
#pragma unroll
        for (int j = 0; j < V; ++j) shift[j] = k.v[j];
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)kBnRowsPerThread * R) {
          Row<T, V> t[kBnRowsPerThread];
          int bi[kBnRowsPerThread];
#pragma unroll
          for (int i = 0; i < kBnRowsPerThread; ++i) {
            const int64_t r = min(rb + (int64_t)i * R, r1 - 1);
            t[i] = load_row<T, V>(xp + r * c);
            bi[i] = pure ? b : batch_row[r];
          }
#pragma unroll
          for (int i = 0; i < kBnRowsPerThread; ++i) {
            const bool take = rb + (int64_t)i * R < r1 && bi[i] == b;
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float d = take ? t[i].v[j] - shift[j] : 0.f;
              s1[j] += d;
              s2[j] = fmaf(d, d, s2[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
          s_red[(rl * 2 + 0) * c + p * V + j] = s1[j];
          s_red[(rl * 2 + 1) * c + p * V + j] = s2[j];
          if (rl == 0) s_shift[p * V + j] = shift[j];
        }
      }
    }
    bn_reduce_lanes(s_red, s_out, s_tmp, c, R);
    const float cnt = (float)count;
    const int64_t o = ((int64_t)blockIdx.x * n_batch + b) * c;
    for (int ch = (int)threadIdx.x; ch < c; ch += (int)blockDim.x) {
      const float a = s_out[ch], q = s_out[c + ch];
      const float m = a / cnt;
      part_mean[o + ch] = s_shift[ch] + m;
      part_m2[o + ch] = clamp_neg(q - a * m);
    }
    if (threadIdx.x == 0) part_cnt[(int64_t)blockIdx.x * n_batch + b] = cnt;
    __syncthreads();   // s_out / s_shift are rewritten for the next instance
  }
}

// One wave per (instance b, channel): lane l takes chunks l, l + 64, ... (kBnMaxChunks / 64 per lane, all requested before
// use); only the chunks whose count for b is positive hold values (the others were never written: selected away, never
// multiplied).  Every chunk mean is taken relative to ONE shift, the mean of the first chunk that holds rows of b, so the
// merge is three weighted sums (k_bn_final's second form), added lane by lane and across lanes in a fixed shuffle tree.
// An instance without rows on this map: mean = 0, rstd = 1 / sqrt(eps).
__global__ __launch_bounds__(256) void k_in_final(const float *__restrict__ part_mean, const float *__restrict__ part_m2,
                                                 const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                 float eps, float *__restrict__ mean_out, float *__restrict__ rstd_out) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b, channel)
  if (idx >= (int64_t)n_batch * c) return;  // whole wave
  const int b = (int)(idx / c), ch = (int)(idx % c);
  constexpr int L = kBnMaxChunks / 64;
  float pn[L], pm[L], pq[L];
  int first = INT_MAX;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int g = lane + i * 64;
    const int64_t gc = min(g, chunks - 1);
    pn[i] = part_cnt[gc * n_batch + b];
    pm[i] = part_mean[(gc * n_batch + b) * c + ch];
    pq[i] = part_m2[(gc * n_batch + b) * c + ch];
  }
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int g = lane + i * 64;
    if (g >= chunks) pn[i] = 0.f;
    if (pn[i] > 0.f) first = min(first, g);
  }
  first = wave_min(first);
  if (first == INT_MAX) {   // whole wave
    if (lane == 0) {
      mean_out[idx] = 0.f;
      rstd_out[idx] = 1.f / sqrtf(eps);
    }
    return;
  }
  const float shift = part_mean[((int64_t)first * n_batch + b) * c + ch];
  float sa = 0.f, sb = 0.f, sn = 0.f;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const bool have = pn[i] > 0.f;
    const float d = have ? pm[i] - shift : 0.f;
    sa = fmaf(pn[i], d, sa);
    sb += have ? fmaf(pn[i] * d, d, pq[i]) : 0.f;
    sn += pn[i];
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {  // lane l absorbs lane l + off: a fixed tree
    const float ta = __shfl_down(sa, off, 64), tb = __shfl_down(sb, off, 64), tn = __shfl_down(sn, off, 64);
    if ((lane & (2 * off - 1)) == 0) {
      sa += ta;
      sb += tb;
      sn += tn;
    }
  }
  if (lane != 0) return;
  const float am = sa / sn;
  const float var = clamp_neg(sb - sa * am) / sn;
  mean_out[idx] = shift + am;
  rstd_out[idx] = 1.f / sqrtf(var + eps);
}

// y = (x - mean[b]) * (rstd[b] * gamma) + beta, b = batch_row[row] (gamma / beta may be NULL: 1 / 0).  k_bn_apply's
// layout: all row loads of a thread first, unconditionally (rows clamped to the matrix), only the stores predicated.  The
// statistics of an instance (a few KB in all, L2-resident) are re-read only when the batch index changes between two
// consecutive rows of the thread.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_in_apply(const T *__restrict__ x, const int32_t *__restrict__ batch_row,
                                                 int64_t n, int c, int n_batch, const float *__restrict__ mean,
                                                 const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                 const float *__restrict__ beta, T *__restrict__ y) {
  const int P = c / V;
  const int W = min(P, (int)blockDim.x);
  const int R = max(1, (int)blockDim.x / P);
  const int rl = (int)threadIdx.x / W;
  const int64_t r0 = (int64_t)blockIdx.x * R * kBnRowsPerThread;
  if (rl >= R) return;
  for (int p = (int)threadIdx.x % W; p < P; p += W) {
    Row<T, V> t[kBnRowsPerThread];
    int bi[kBnRowsPerThread];
#pragma unroll
    for (int i = 0; i < kBnRowsPerThread; ++i) {
      const int64_t r = min(r0 + rl + (int64_t)i * R, n - 1);
      t[i] = load_row<T, V>(x + r * c + p * V);
      bi[i] = min(max(batch_row[r], 0), n_batch - 1);
    }
    float ga[V], be[V], a[V], mu[V];
    load_affine<V>(gamma, beta, p * V, ga, be);
#pragma unroll
    for (int i = 0; i < kBnRowsPerThread; ++i) {
      const int64_t r = r0 + rl + (int64_t)i * R;
      if (i == 0 || bi[i] != bi[i - 1]) {
        load_f32<V>(mean + (int64_t)bi[i] * c + p * V, mu);
        load_f32<V>(rstd + (int64_t)bi[i] * c + p * V, a);
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] *= ga[j];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) t[i].v[j] = fmaf(t[i].v[j] - mu[j], a[j], be[j]);
      if (r < n) store_row<T, V>(y + r * c + p * V, t[i]);
    }
  }
}

// per (chunk, instance, channel): sum dy and sum dy * xhat (xhat = (x - mean[b]) * rstd[b]); layout of k_in_partial
template <typename T, int V>
__global__ __launch_bounds__(256) void k_in_bwd_partial(const T *__restrict__ x, const T *__restrict__ dy,
                                                       const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                       int chunks, int n_batch, const float *__restrict__ mean,
                                                       const float *__restrict__ rstd, float *__restrict__ part_dy,
                                                       float *__restrict__ part_dyx, float *__restrict__ part_cnt) {
  extern __shared__ float s_red[];  // in_partial_lds_bytes
  const int P = c / V;
  const int W = min(P, (int)blockDim.x);
  const int R = max(1, (int)blockDim.x / P);
  float *s_out = s_red + (size_t)R * 2 * c, *s_tmp = s_out + 2 * c;
  int *s_i = reinterpret_cast<int *>(s_tmp);
  const int64_t r0 = chunk_begin(blockIdx.x, n, chunks), r1 = chunk_begin(blockIdx.x + 1, n, chunks);
  if (r0 >= r1) return;  // whole workgroup
  int bmin, bmax;
  in_scan_range(batch_row, r0, r1, n_batch, s_i, bmin, bmax);
  const bool pure = bmin == bmax;
  constexpr int RB = kBnRowsPerThread / 2;   // rows in flight per thread (x and dy: 8 loads)
  for (int b = bmin; b <= bmax; ++b) {
    int first = 0, count = (int)(r1 - r0);
    if (!pure) {
      in_scan_instance(batch_row, r0, r1, b, s_i + 2, first, count);
      if (count == 0) {   // uniform
        __syncthreads();
        continue;
      }
    }
    for (int p0 = 0; p0 < P; p0 += blockDim.x) {
      const int p = p0 + (int)threadIdx.x % W;
      const int rl = (int)threadIdx.x / W;
      const bool active = rl < R && p < P;
      float s1[V], s2[V];
#pragma unroll
      for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
      if (active) {
        float m[V], rs[V];
        load_f32<V>(mean + (int64_t)b * c + p * V, m);
        load_f32<V>(rstd + (int64_t)b * c + p * V, rs);
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)RB * R) {
          Row<T, V> tx[RB], tg[RB];
          int bi[RB];
#pragma unroll
          for (int i = 0; i < RB; ++i) {
            const int64_t r = min(rb + (int64_t)i * R, r1 - 1);
            tx[i] = load_row<T, V>(x + r * c + p * V);
            tg[i] = load_row<T, V>(dy + r * c + p * V);
            bi[i] = pure ? b : batch_row[r];
          }
#pragma unroll
          for (int i = 0; i < RB; ++i) {
            const bool take = rb + (int64_t)i * R < r1 && bi[i] == b;
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float xh = (tx[i].v[j] - m[j]) * rs[j];
              const float g = take ? tg[i].v[j] : 0.f;
              s1[j] += g;
              s2[j] = fmaf(g, take ? xh : 0.f, s2[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
          s_red[(rl * 2 + 0) * c + p * V + j] = s1[j];
          s_red[(rl * 2 + 1) * c + p * V + j] = s2[j];
        }
      }
    }
    bn_reduce_lanes(s_red, s_out, s_tmp, c, R);
    const int64_t o = ((int64_t)blockIdx.x * n_batch + b) * c;
    for (int ch = (int)threadIdx.x; ch < c; ch += (int)blockDim.x) {
      part_dy[o + ch] = s_out[ch];
      part_dyx[o + ch] = s_out[c + ch];
    }
    if (threadIdx.x == 0) part_cnt[(int64_t)blockIdx.x * n_batch + b] = (float)count;
    __syncthreads();
  }
}

// sums of the chunks per (instance, channel) in a fixed order (one wave each, as k_in_final): t1 = sum dy,
// t2 = sum dy * xhat, rows[b] = rows of the instance
__global__ __launch_bounds__(256) void k_in_bwd_final(const float *__restrict__ part_dy,
                                                     const float *__restrict__ part_dyx,
                                                     const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                     float *__restrict__ t1, float *__restrict__ t2,
                                                     float *__restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= (int64_t)n_batch * c) return;  // whole wave
  const int b = (int)(idx / c), ch = (int)(idx % c);
  constexpr int L = kBnMaxChunks / 64;
  float pn[L], pa[L], pb[L];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int g = lane + i * 64;
    const int64_t gc = min(g, chunks - 1);
    pn[i] = part_cnt[gc * n_batch + b];
    pa[i] = part_dy[(gc * n_batch + b) * c + ch];
    pb[i] = part_dyx[(gc * n_batch + b) * c + ch];
  }
  float a = 0.f, q = 0.f, sn = 0.f;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const bool have = lane + i * 64 < chunks && pn[i] > 0.f;
    a += have ? pa[i] : 0.f;
    q += have ? pb[i] : 0.f;
    sn += have ? pn[i] : 0.f;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float ta = __shfl_down(a, off, 64), tq = __shfl_down(q, off, 64), tn = __shfl_down(sn, off, 64);
    if ((lane & (2 * off - 1)) == 0) {
      a += ta;
      q += tq;
      sn += tn;
    }
  }
  if (lane == 0) {
    t1[idx] = a;
    t2[idx] = q;
    if (ch == 0) rows[b] = sn;
  }
}

// grad_beta = sum over the instances (ascending) of t1, grad_gamma = of t2; either may be NULL
__global__ __launch_bounds__(256) void k_in_bwd_params(const float *__restrict__ t1, const float *__restrict__ t2,
                                                      int n_batch, int c, float *__restrict__ grad_gamma,
                                                      float *__restrict__ grad_beta) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  float a = 0.f, q = 0.f;
  for (int b = 0; b < n_batch; ++b) {
    a += t1[(int64_t)b * c + ch];
    q += t2[(int64_t)b * c + ch];
  }
  if (grad_beta != nullptr) grad_beta[ch] = a;
  if (grad_gamma != nullptr) grad_gamma[ch] = q;
}

// dx = A * ((dy - k1) - (x - mean[b]) * k2) with A = gamma * rstd[b], k1 = t1[b] / n_b, k2 = t2[b] / n_b * rstd[b]
// (layout and coefficient reuse of k_in_apply)
template <typename T, int V>
__global__ __launch_bounds__(256) void k_in_bwd_apply(const T *__restrict__ x, const T *__restrict__ dy,
                                                     const int32_t *__restrict__ batch_row, int64_t n, int c,
                                                     int n_batch, const float *__restrict__ mean,
                                                     const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                     const float *__restrict__ t1, const float *__restrict__ t2,
                                                     const float *__restrict__ rows, T *__restrict__ dx) {
  const int P = c / V;
  const int W = min(P, (int)blockDim.x);
  const int R = max(1, (int)blockDim.x / P);
  const int rl = (int)threadIdx.x / W;
  constexpr int RB = kBnRowsPerThread;
  const int64_t r0 = (int64_t)blockIdx.x * R * RB;
  if (rl >= R) return;
  for (int p = (int)threadIdx.x % W; p < P; p += W) {
    Row<T, V> tx[RB], tg[RB];
    int bi[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int64_t r = min(r0 + rl + (int64_t)i * R, n - 1);
      tx[i] = load_row<T, V>(x + r * c + p * V);
      tg[i] = load_row<T, V>(dy + r * c + p * V);
      bi[i] = min(max(batch_row[r], 0), n_batch - 1);
    }
    float ga[V], unused[V], A[V], k1[V], k2[V], mu[V];
    load_affine<V>(gamma, nullptr, p * V, ga, unused);
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int64_t r = r0 + rl + (int64_t)i * R;
      if (i == 0 || bi[i] != bi[i - 1]) {
        const int64_t o = (int64_t)bi[i] * c + p * V;
        const float inv_n = 1.f / fmaxf(rows[bi[i]], 1.f);
        load_f32<V>(mean + o, mu);
        load_f32<V>(rstd + o, A);
        load_f32<V>(t1 + o, k1);
        load_f32<V>(t2 + o, k2);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          k1[j] *= inv_n;
          k2[j] *= inv_n * A[j];
          A[j] *= ga[j];
        }
      }
      Row<T, V> out;
#pragma unroll
      for (int j = 0; j < V; ++j) out.v[j] = A[j] * ((tg[i].v[j] - k1[j]) - (tx[i].v[j] - mu[j]) * k2[j]);
      if (r < n) store_row<T, V>(dx + r * c + p * V, out);
    }
  }
}

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
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  double a = 0.0, q = 0.0;
  for (int b = 0; b < n_batch; ++b) {
    a += t1[(int64_t)b * c + ch];
    q += t2[(int64_t)b * c + ch];
  }
  if (grad_beta != nullptr) grad_beta[ch] = a;
  if (grad_gamma != nullptr) grad_gamma[ch] = q;
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
// workspace: part_a | part_b [chunks][n_batch][c] floats | part_cnt [chunks][n_batch] | t1 | t2 [n_batch][c] | rows [n_batch]
// (every piece 256-byte aligned; the float64 entry points use t1 | t2 | rows as doubles at the start)
struct InWs {
  float *pa, *pb, *cnt, *t1, *t2, *rows;
};
static int64_t in_ws_layout(int64_t n, int n_batch, int c, char *base, InWs *w) {
  const int64_t chunks = bn_chunks_max(n);
  const int64_t part = align_up(chunks * n_batch * c * 4, 256), pc = align_up(chunks * n_batch * 4, 256);
  const int64_t t = align_up((int64_t)n_batch * c * 4, 256), rw = align_up((int64_t)n_batch * 4, 256);
  if (w != nullptr) {
    w->pa = reinterpret_cast<float *>(base);
    w->pb = reinterpret_cast<float *>(base + part);
    w->cnt = reinterpret_cast<float *>(base + 2 * part);
    w->t1 = reinterpret_cast<float *>(base + 2 * part + pc);
    w->t2 = reinterpret_cast<float *>(base + 2 * part + pc + t);
    w->rows = reinterpret_cast<float *>(base + 2 * part + pc + 2 * t);
  }
  const int64_t f32 = 2 * part + pc + 2 * t + rw;
  const int64_t f64 = 2 * align_up((int64_t)n_batch * c * 8, 256) + align_up((int64_t)n_batch * 8, 256);
  return f32 > f64 ? f32 : f64;
}

// widest piece for rows of c channels of T when every address is 16-byte aligned (as bn_stats): 16 bytes, else 4 elements
template <typename T>
static int in_piece(int c, std::initializer_list<const void *> ptrs) {
  constexpr int W = 16 / (int)sizeof(T);
  bool aligned = true;
  for (const void *p : ptrs) aligned = aligned && (uintptr_t)p % 16 == 0;
  return (aligned && c % W == 0) ? W : ((aligned && c % 4 == 0) ? 4 : 1);
}

#define ME_IN_DISPATCH_V(T, v, ...)                            \
  do {                                                         \
    constexpr int W_ = 16 / (int)sizeof(T);                    \
    if ((v) == W_) { constexpr int V = W_; __VA_ARGS__; }      \
    else if ((v) == 4) { constexpr int V = 4; __VA_ARGS__; }   \
    else { constexpr int V = 1; __VA_ARGS__; }                 \
  } while (0)

template <typename T>
static int in_stats(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, float eps, float *mean,
                    float *rstd, const InWs &w, hipStream_t stream) {
  const int v = in_piece<T>(c, {x});
  const int P = c / v;
  const int R = P >= 256 ? 1 : 256 / P;
  const int chunks = bn_chunks(n, R, kBnRowsPerThread);
  const size_t lds = in_partial_lds_bytes(c, R);
  ME_CHECK(lds <= 64 * 1024, "channel count too large for the instance-norm kernels");
  ME_HIP(hipMemsetAsync(w.cnt, 0, (size_t)chunks * n_batch * 4, stream));
  if (n > 0)
    ME_IN_DISPATCH_V(T, v, hipLaunchKernelGGL((k_in_partial<T, V>), dim3(chunks), dim3(256), lds, stream, x, batch_row, n,
                                              c, chunks, n_batch, w.pa, w.pb, w.cnt));
  hipLaunchKernelGGL(k_in_final, dim3((unsigned)ceil_div((int64_t)n_batch * c, 4)), dim3(256), 0, stream, w.pa, w.pb,
                     w.cnt, chunks, n_batch, c, eps, mean, rstd);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int in_apply(const T *x, const int32_t *batch_row, int64_t n, int n_batch, int c, const float *mean,
                    const float *rstd, const float *gamma, const float *beta, T *y, hipStream_t stream) {
  const int v = in_piece<T>(c, {x, y, mean, rstd});
  const int P = c / v;
  const dim3 grid((unsigned)ceil_div(n, (int64_t)(P >= 256 ? 1 : 256 / P) * kBnRowsPerThread));
  ME_IN_DISPATCH_V(T, v, hipLaunchKernelGGL((k_in_apply<T, V>), grid, dim3(256), 0, stream, x, batch_row, n, c, n_batch,
                                            mean, rstd, gamma, beta, y));
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int in_backward(const T *x, const T *dy, const int32_t *batch_row, int64_t n, int n_batch, int c,
                       const float *mean, const float *rstd, const float *gamma, T *dx, float *grad_gamma,
                       float *grad_beta, const InWs &w, hipStream_t stream) {
  const int v = in_piece<T>(c, {x, dy, dx, mean, rstd});
  const int P = c / v;
  const int R = P >= 256 ? 1 : 256 / P;
  const int chunks = bn_chunks(n, R, kBnRowsPerThread / 2);
  const size_t lds = in_partial_lds_bytes(c, R);
  ME_CHECK(lds <= 64 * 1024, "channel count too large for the instance-norm kernels");
  ME_HIP(hipMemsetAsync(w.cnt, 0, (size_t)chunks * n_batch * 4, stream));
  ME_IN_DISPATCH_V(T, v, hipLaunchKernelGGL((k_in_bwd_partial<T, V>), dim3(chunks), dim3(256), lds, stream, x, dy,
                                            batch_row, n, c, chunks, n_batch, mean, rstd, w.pa, w.pb, w.cnt));
  hipLaunchKernelGGL(k_in_bwd_final, dim3((unsigned)ceil_div((int64_t)n_batch * c, 4)), dim3(256), 0, stream, w.pa, w.pb,
                     w.cnt, chunks, n_batch, c, w.t1, w.t2, w.rows);
  if (grad_gamma != nullptr || grad_beta != nullptr)
    hipLaunchKernelGGL(k_in_bwd_params, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, stream, w.t1, w.t2, n_batch, c,
                       grad_gamma, grad_beta);
  if (dx != nullptr) {
    const dim3 grid((unsigned)ceil_div(n, (int64_t)R * kBnRowsPerThread));
    ME_IN_DISPATCH_V(T, v, hipLaunchKernelGGL((k_in_bwd_apply<T, V>), grid, dim3(256), 0, stream, x, dy, batch_row, n, c,
                                              n_batch, mean, rstd, gamma, w.t1, w.t2, w.rows, dx));
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
  if (is_bf16)
    return in_stats<__bf16>(reinterpret_cast<const __bf16 *>(x), batch_row, n, n_batch, c, eps, mean, rstd, w, stream);
  return in_stats<float>(reinterpret_cast<const float *>(x), batch_row, n, n_batch, c, eps, mean, rstd, w, stream);
}

int me_inorm_apply(const void *x, int32_t is_bf16, const int32_t *batch_row, int64_t n, int32_t n_batch, int32_t c,
                   const float *mean, const float *rstd, const float *gamma, const float *beta, void *y,
                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_IN_CHECK_ARGS();
  if (n == 0) return 0;
  if (is_bf16)
    return in_apply<__bf16>(reinterpret_cast<const __bf16 *>(x), batch_row, n, n_batch, c, mean, rstd, gamma, beta,
                            reinterpret_cast<__bf16 *>(y), stream);
  return in_apply<float>(reinterpret_cast<const float *>(x), batch_row, n, n_batch, c, mean, rstd, gamma, beta,
                         reinterpret_cast<float *>(y), stream);
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
  if (is_bf16)
    return in_backward<__bf16>(reinterpret_cast<const __bf16 *>(x), reinterpret_cast<const __bf16 *>(dy), batch_row, n,
                               n_batch, c, mean, rstd, gamma, reinterpret_cast<__bf16 *>(dx), grad_gamma, grad_beta, w,
                               stream);
  return in_backward<float>(reinterpret_cast<const float *>(x), reinterpret_cast<const float *>(dy), batch_row, n,
                            n_batch, c, mean, rstd, gamma, reinterpret_cast<float *>(dx), grad_gamma, grad_beta, w,
                            stream);
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
