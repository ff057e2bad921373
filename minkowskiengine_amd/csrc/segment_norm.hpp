// Shared by the normalisations whose statistics are SEGMENTED by the batch index of each row (instance_norm.hip: one
// record per (instance, channel); group_norm.hip: the channel records of a group merged into one): the scans of a chunk
// of rows, the bodies of the two-level reductions over (chunk, instance, channel) and the workspace they use — a
// translation unit wraps each body in a __global__ kernel of its own — and seg_rows / k_seg_rows, the row tile of every
// apply and backward-apply kernel, which a translation unit instantiates with its maps.  Host side: the workspace and
// the launch of seg_rows over a plan (SegPlan, norm_common.hpp).
#pragma once
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
// host — only the (g, b) with rows are written, and only those are read by the second level.
// Thread layout and load-first structure of k_bn_partial (norm.hip): P = c / V pieces per row, R row lanes, every load of a
// batch of rows unconditional (row clamped to the chunk) with the contribution selected afterwards.
// s_red: the kernel's dynamic LDS, in_partial_lds_bytes.
template <typename T, int V>
__device__ __forceinline__ void seg_partial(float *s_red, const T *__restrict__ x,
                                            const int32_t *__restrict__ batch_row, int64_t n, int c, int chunks,
                                            int n_batch, float *__restrict__ part_mean, float *__restrict__ part_m2,
                                            float *__restrict__ part_cnt) {
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
        const Piece<V> k = load_piece<T, V>(xp + (r0 + first) * c);
#pragma unroll
        for (int j = 0; j < V; ++j) shift[j] = k.v[j];
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)kBnRowsPerThread * R) {
          Piece<V> t[kBnRowsPerThread];
          int bi[kBnRowsPerThread];
#pragma unroll
          for (int i = 0; i < kBnRowsPerThread; ++i) {
            const int64_t r = min(rb + (int64_t)i * R, r1 - 1);
            t[i] = load_piece<T, V>(xp + r * c);
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

// The record of (instance b, channel ch) from its chunk records, by one wave: lane l takes chunks l, l + 64, ...
// (kBnMaxChunks / 64 per lane, all requested before use); only the chunks whose count for b is positive hold values (the
// others were never written: selected away, never multiplied).  Every chunk mean is taken relative to ONE shift, the mean
// of the first chunk that holds rows of b, so the merge is three weighted sums (k_bn_final's second form), added lane by
// lane and across lanes in a fixed shuffle tree.  -> false (whole wave) for an instance without rows on this map; else
// lane 0 holds the record as rows, shift + am = mean and sb - sa * am = M2.
struct SegMerge {
  float shift, sa, sb, sn;
};
__device__ __forceinline__ bool seg_merge_chunks(const float *__restrict__ part_mean, const float *__restrict__ part_m2,
                                                 const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                                 int b, int ch, SegMerge &out) {
  const int lane = threadIdx.x & 63;
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
  if (first == INT_MAX) return false;   // whole wave
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
  out.shift = shift;
  out.sa = sa;
  out.sb = sb;
  out.sn = sn;
  return true;
}

// the gradient that seg_bwd_partial sums is dy itself (instance norm, group norm)
struct SegGradPlain {
  template <int V>
  struct State {};
  template <int V>
  __device__ __forceinline__ void load(int, int, const float (&)[V], State<V> &) const {}
  template <int V>
  __device__ __forceinline__ float operator()(const State<V> &, int, float, float g) const {
    return g;
  }
};

// per (chunk, instance, channel): sum dy and sum dy * xhat (xhat = (x - mean) * rstd); layout of seg_partial.
// coef(b, ch0, m, rs) loads the mean and rstd of instance b for the V channels from ch0, once per (instance, piece).
// grad maps dy to the gradient that is summed (default: dy): grad.load(b, ch0, rs, st) fills its coefficients of
// (instance, piece) next to mean and rstd, grad(st, j, x - mean, dy) is the value of element j.
template <typename T, int V, typename Coef, typename Grad = SegGradPlain>
__device__ __forceinline__ void seg_bwd_partial(float *s_red, const T *__restrict__ x, const T *__restrict__ dy,
                                                const int32_t *__restrict__ batch_row, int64_t n, int c, int chunks,
                                                int n_batch, const Coef &coef, float *__restrict__ part_dy,
                                                float *__restrict__ part_dyx, float *__restrict__ part_cnt,
                                                const Grad &grad = Grad()) {
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
        coef(b, p * V, m, rs);
        typename Grad::template State<V> st;
        grad.template load<V>(b, p * V, rs, st);
        for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)RB * R) {
          Piece<V> tx[RB], tg[RB];
          int bi[RB];
#pragma unroll
          for (int i = 0; i < RB; ++i) {
            const int64_t r = min(rb + (int64_t)i * R, r1 - 1);
            tx[i] = load_piece<T, V>(x + r * c + p * V);
            tg[i] = load_piece<T, V>(dy + r * c + p * V);
            bi[i] = pure ? b : batch_row[r];
          }
#pragma unroll
          for (int i = 0; i < RB; ++i) {
            const bool take = rb + (int64_t)i * R < r1 && bi[i] == b;
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float xh = (tx[i].v[j] - m[j]) * rs[j];
              const float g = take ? grad(st, j, tx[i].v[j] - m[j], tg[i].v[j]) : 0.f;
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

// sums of the chunks per (instance, channel) in a fixed order (one wave each, as seg_merge_chunks): t1 = sum dy,
// t2 = sum dy * xhat, rows[b] = rows of the instance
__device__ __forceinline__ void seg_bwd_final(const float *__restrict__ part_dy, const float *__restrict__ part_dyx,
                                              const float *__restrict__ part_cnt, int chunks, int n_batch, int c,
                                              float *__restrict__ t1, float *__restrict__ t2, float *__restrict__ rows) {
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

// grad_beta = sum over the instances (ascending) of t1, grad_gamma = of t2; either may be NULL (F: float or double)
template <typename F>
__device__ __forceinline__ void seg_bwd_params(const F *__restrict__ t1, const F *__restrict__ t2, int n_batch, int c,
                                               F *__restrict__ grad_gamma, F *__restrict__ grad_beta) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  F a = 0, q = 0;
  for (int b = 0; b < n_batch; ++b) {
    a += t1[(int64_t)b * c + ch];
    q += t2[(int64_t)b * c + ch];
  }
  if (grad_beta != nullptr) grad_beta[ch] = a;
  if (grad_gamma != nullptr) grad_gamma[ch] = q;
}

// The row tile of every kernel that maps rows to rows with coefficients per instance (the apply and the backward-apply
// kernels): out[r] = map(x[r][, dy[r]]) with the coefficients of b = batch_row[r].  k_bn_apply's layout: a thread owns a
// piece of V channels and kBnRowsPerThread rows; ALL its row loads are issued first and unconditionally (rows clamped to
// the matrix), only the stores are predicated.  The batch index is clamped to [0, n_batch) before anything is addressed
// with it.  The coefficients of an instance (a few KB in all, L2-resident) are re-read only when the batch index changes
// between two consecutive rows of the thread.  Map (passed by value as a kernel argument) provides
//   kDy                       whether the map reads dy next to x
//   Piece<V>                  the registers of a thread's piece
//   init(ch0, pc)             once per piece, outside the row loop: what depends on the channels only
//   load(b, ch0, pc)          at a change of the batch index: the coefficients of instance b
//   value(pc, j, x[, dy])     element j of the piece
template <typename T, int V, typename Map>
__device__ __forceinline__ void seg_rows(const T *__restrict__ x, const T *__restrict__ dy,
                                         const int32_t *__restrict__ batch_row, int64_t n, int c, int n_batch,
                                         const Map &map, T *__restrict__ out) {
  const int P = c / V;
  const int W = min(P, (int)blockDim.x);
  const int R = max(1, (int)blockDim.x / P);
  const int rl = (int)threadIdx.x / W;
  constexpr int RB = kBnRowsPerThread;
  const int64_t r0 = (int64_t)blockIdx.x * R * RB;
  if (rl >= R) return;
  for (int p = (int)threadIdx.x % W; p < P; p += W) {
    Piece<V> tx[RB], tg[Map::kDy ? RB : 1];
    int bi[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int64_t r = min(r0 + rl + (int64_t)i * R, n - 1);
      tx[i] = load_piece<T, V>(x + r * c + p * V);
      if constexpr (Map::kDy) tg[i] = load_piece<T, V>(dy + r * c + p * V);
      bi[i] = min(max(batch_row[r], 0), n_batch - 1);
    }
    typename Map::template Piece<V> pc;
    map.template init<V>(p * V, pc);
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int64_t r = r0 + rl + (int64_t)i * R;
      if (i == 0 || bi[i] != bi[i - 1]) map.template load<V>(bi[i], p * V, pc);
      Piece<V> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if constexpr (Map::kDy) o.v[j] = map.template value<V>(pc, j, tx[i].v[j], tg[i].v[j]);
        else o.v[j] = map.template value<V>(pc, j, tx[i].v[j]);
      }
      if (r < n) store_piece<T, V>(out + r * c + p * V, o);
    }
  }
}
// dy is NULL for a map that does not read it
template <typename T, int V, typename Map>
__global__ __launch_bounds__(256) void k_seg_rows(const T *__restrict__ x, const T *__restrict__ dy,
                                                 const int32_t *__restrict__ batch_row, int64_t n, int c, int n_batch,
                                                 const Map map, T *__restrict__ out) {
  seg_rows<T, V, Map>(x, dy, batch_row, n, c, n_batch, map, out);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// workspace: part_a | part_b [chunks][n_batch][c] floats | part_cnt [chunks][n_batch] | t1 | t2 [n_batch][c] | rows [n_batch]
// (every piece 256-byte aligned).  -> bytes of the fp32 layout
struct InWs {
  float *pa, *pb, *cnt, *t1, *t2, *rows;
};
static int64_t in_ws_layout_f32(int64_t n, int n_batch, int c, char *base, InWs *w) {
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
  return 2 * part + pc + 2 * t + rw;
}

// seg_rows over the plan's grid with the map `map`; dy is NULL for a map that does not read it
#define ME_SEG_ROWS(T, pl, stream, x, dy, batch_row, n, c, n_batch, map, out)                                     \
  ME_PIECE_DISPATCH(T, kPieceNorm, (pl).v,                                                                        \
                    hipLaunchKernelGGL((k_seg_rows<T, V, std::decay_t<decltype(map)>>), (pl).grid, dim3(256), 0, \
                                       stream, x, dy, batch_row, n, c, n_batch, map, out))

}  // namespace me
