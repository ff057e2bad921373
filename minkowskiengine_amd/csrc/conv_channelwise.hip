// Channelwise (depthwise) convolution for gfx950 (MI355X): every channel has its own kernel, W is [volume, c].
//
// The reference's MinkowskiChannelwiseConvolution (MinkowskiEngine/MinkowskiChannelwiseConvolution.py:184-189) is
// plain Python: one gather, multiply and index_put per kernel offset, the backward left to autograd over advanced
// indexing.  It has no native operator.  Here the maths is a WEIGHTED local sum pooling on the dense neighbour tables
// the convolution and pooling already use (nbr = tbl[k][out row] -> in row or -1, nbrT = its transpose):
//
//   y[t, c]  = bias[c] + sum_k W[k, c] * x[nbr[k, t], c]          k_cw_forward     (target-stationary on nbr)
//   dx[i, c] = sum_k W[k, c] * dy[nbrT[k, i], c]                    k_cw_backward_partial (DX) or k_cw_forward on nbrT
//   dW[k, c] = sum_i x[i, c] * dy[nbrT[k, i], c]                    k_cw_backward_partial + k_cw_backward_final
//   db[c]    = sum_t dy[t, c]                                       (same two kernels, extra columns)
//
// Forward: a thread owns a (target row, 16-byte channel piece) as in pool.hip, walks k in ascending order with fp32
// fmaf, adds the bias and writes its piece once: no atomics, no zero fill, rows without neighbours get the bias (or 0).
// Backward: a thread owns a (source row, channel piece) of a chunk of rows and loads x[i] once; for each k of its
// k-group it gathers g = dy[nbrT[k, i]], adds x[i] * g to that k's register partial and W[k] * g to dx[i].  The
// partials of a workgroup's row lanes are added in lane order through LDS (one partial row per chunk and k), then
// k_cw_backward_final adds the chunks in a fixed order.  Every sum has a fixed order: bitwise reproducible.
//
// Volume: the backward keeps KG per-k partials in registers (KG * V floats per thread, KG = 16 for 4-channel pieces and
// 32 for single channels).  A larger volume runs in
// k-groups of KG (grid.y); then dx is a separate target-stationary pass (k_cw_forward on nbrT, no bias), which gives
// the same bits as the fused one.  So the volume is bounded only by the table's int32 indexing: volume <= 65535 as in
// pool.hip, an error beyond it.
//
// bf16 features take fp32 weights and bias (the fp32 master weights of convolution.py), accumulate in fp32 and round
// once at the store; dW and db are fp32 for every feature type but double.
#include "piece.hpp"

namespace me {
namespace cw {

// Offsets per batch of the gathers: the KB table entries of a batch are requested together, then the KB feature pieces
// (an absent neighbour, -1, reads row 0 — a valid row whenever the source has one — and its value is not used), then
// they are added in k order.  One table load, a wait, one gather and a wait per offset left every thread with one load
// in flight: 67 us for 100k x 64 fp32 at 3^3 (0.15 of the byte model's HBM time).
constexpr int KB = 8;

// dst[t] = bias + sum_k w[k] * src[tbl[k][t]]   (bias may be NULL; the input gradient: tbl = nbrT, bias NULL)
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cw_forward(const T *__restrict__ src, int c, const float *__restrict__ w,
                                                   const float *__restrict__ bias, const int32_t *__restrict__ tbl,
                                                   int64_t n_src, int64_t n_tgt, int volume, T *__restrict__ dst) {
  const int pieces = c / V;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_tgt * pieces) return;
  const int64_t t = idx / pieces;
  const int ch = (int)(idx % pieces) * V;
  Piece<V> acc;
#pragma unroll
  for (int j = 0; j < V; ++j) acc.v[j] = 0.f;
  const int vol = n_src > 0 ? volume : 0;   // (no source rows: every entry is -1 and row 0 does not exist)
  for (int k0 = 0; k0 < vol; k0 += KB) {
    int32_t s[KB];
#pragma unroll
    for (int b = 0; b < KB; ++b) s[b] = tbl[(int64_t)min(k0 + b, vol - 1) * n_tgt + t];
    Piece<V> x[KB];
#pragma unroll
    for (int b = 0; b < KB; ++b) x[b] = load_piece<T, V>(src + (int64_t)(s[b] < 0 ? 0 : s[b]) * c + ch);
#pragma unroll
    for (int b = 0; b < KB; ++b) {
      if (k0 + b < vol && s[b] >= 0) {
        Piece<V> wk;
        load_f32<V>(w + (int64_t)(k0 + b) * c + ch, wk.v);
#pragma unroll
        for (int j = 0; j < V; ++j) acc.v[j] = fmaf(wk.v[j], x[b].v[j], acc.v[j]);
      }
    }
  }
  if (bias) {
    Piece<V> b;
    load_f32<V>(bias + ch, b.v);
#pragma unroll
    for (int j = 0; j < V; ++j) acc.v[j] += b.v[j];
  }
  store_piece<T, V>(dst + t * c + ch, acc);
}

// Workgroup (chunk g = blockIdx.x, k-group blockIdx.y: offsets [k0, k0 + KG) of the volume).  Pieces of a row:
// P = c / V; the 256 threads are PB = min(P, 256) pieces x R = 256 / PB row lanes; lane rl takes rows r0 + rl,
// r0 + rl + R, ... of the chunk (more than 256 pieces: a loop over blocks of 256).
// part[g][q]: q = k * c + channel for dW, q = volume * c + channel for db (k-group 0 only, rows of dy).
// DX (one k-group covers the volume): dx[i] = sum_k w[k] * dy[nbrT[k][i]] is written on the way.
template <typename T, int V, int KG, bool DX>
__global__ __launch_bounds__(256) void k_cw_backward_partial(const T *__restrict__ x, const T *__restrict__ dy, int c,
                                                            const float *__restrict__ w,
                                                            const int32_t *__restrict__ tbl_t, int64_t n_in,
                                                            int64_t n_out, int volume, int chunks, int has_db,
                                                            T *__restrict__ dx, float *__restrict__ part) {
  __shared__ float s_red[256 * V];
  const int P = c / V;
  const int PB = P < 256 ? P : 256;
  const int R = 256 / PB;
  const int tp = (int)threadIdx.x % PB, rl = (int)threadIdx.x / PB;
  const int64_t g = blockIdx.x;
  const int k0 = (int)blockIdx.y * KG, k1 = min(volume, k0 + KG);
  const int64_t ncol = (int64_t)volume * c + c;
  float *pg = part + g * ncol;
  const int64_t r0 = chunk_begin(g, n_in, chunks), r1 = chunk_begin(g + 1, n_in, chunks);

  // the R row lanes' values s_red[rl][q] are added in lane order into out[q], q < valid
  auto reduce_lanes = [&](float *out, int valid) {
    __syncthreads();
    for (int q = (int)threadIdx.x; q < valid; q += 256) {
      float a = 0.f;
      for (int l = 0; l < R; ++l) a += s_red[l * PB * V + q];
      out[q] = a;
    }
    __syncthreads();
  };

  for (int p0 = 0; p0 < P; p0 += PB) {
    const int p = p0 + tp;
    const bool active = rl < R && p < P;
    const int ch = p * V;
    float acc[KG][V];
#pragma unroll
    for (int kk = 0; kk < KG; ++kk)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[kk][j] = 0.f;
    if (active) {
      // (batches of KB offsets as in k_cw_forward: tables, then gathers, then the sums in k order; no output rows:
      // every entry is -1 and nothing is gathered)
      const int kend = n_out > 0 ? k1 : k0;
      for (int64_t i = r0 + rl; i < r1; i += R) {
        const Piece<V> xi = load_piece<T, V>(x + i * c + ch);
        Piece<V> d;
#pragma unroll
        for (int j = 0; j < V; ++j) d.v[j] = 0.f;
#pragma unroll
        for (int kb = 0; kb < KG; kb += KB) {
          if (k0 + kb < kend) {
            int32_t o[KB];
#pragma unroll
            for (int b = 0; b < KB; ++b) o[b] = tbl_t[(int64_t)min(k0 + kb + b, kend - 1) * n_in + i];
            Piece<V> gy[KB];
#pragma unroll
            for (int b = 0; b < KB; ++b) gy[b] = load_piece<T, V>(dy + (int64_t)(o[b] < 0 ? 0 : o[b]) * c + ch);
#pragma unroll
            for (int b = 0; b < KB; ++b) {
              const int k = k0 + kb + b;
              if (k < kend && o[b] >= 0) {
#pragma unroll
                for (int j = 0; j < V; ++j) acc[kb + b][j] = fmaf(xi.v[j], gy[b].v[j], acc[kb + b][j]);
                if constexpr (DX) {
                  Piece<V> wk;
                  load_f32<V>(w + (int64_t)k * c + ch, wk.v);
#pragma unroll
                  for (int j = 0; j < V; ++j) d.v[j] = fmaf(wk.v[j], gy[b].v[j], d.v[j]);
                }
              }
            }
          }
        }
        if constexpr (DX) store_piece<T, V>(dx + i * c + ch, d);
      }
    }
    const int valid = min(PB, P - p0) * V;   // channels of this block of pieces
#pragma unroll
    for (int kk = 0; kk < KG; ++kk) {
      if (k0 + kk < k1) {   // (uniform over the workgroup)
        if (active) {
#pragma unroll
          for (int j = 0; j < V; ++j) s_red[rl * PB * V + tp * V + j] = acc[kk][j];
        }
        reduce_lanes(pg + (int64_t)(k0 + kk) * c + p0 * V, valid);
      }
    }
    if (has_db && blockIdx.y == 0) {
      const int64_t b0 = chunk_begin(g, n_out, chunks), b1 = chunk_begin(g + 1, n_out, chunks);
      Piece<V> s;
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = 0.f;
      if (active) {
        for (int64_t t = b0 + rl; t < b1; t += R) {
          const Piece<V> gy = load_piece<T, V>(dy + t * c + ch);
#pragma unroll
          for (int j = 0; j < V; ++j) s.v[j] += gy.v[j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) s_red[rl * PB * V + tp * V + j] = s.v[j];
      }
      reduce_lanes(pg + (int64_t)volume * c + p0 * V, valid);
    }
  }
}

// dW / db = sum over the chunks in ascending order: 16 columns x 16 chunk lanes per workgroup, lane s takes chunks
// s, s + 16, ...; the 16 lane sums are added in lane order.
__global__ __launch_bounds__(256) void k_cw_backward_final(const float *__restrict__ part, int chunks, int64_t ncol,
                                                          int64_t nw, int has_db, float *__restrict__ dw,
                                                          float *__restrict__ db) {
  __shared__ float s_red[256];
  const int col = (int)threadIdx.x & 15, s = (int)threadIdx.x >> 4;
  const int64_t q = (int64_t)blockIdx.x * 16 + col;
  const int64_t nq = has_db ? ncol : nw;
  float a = 0.f;
  if (q < nq) {
#pragma unroll 8
    for (int gg = s; gg < chunks; gg += 16) a += part[(int64_t)gg * ncol + q];
  }
  s_red[threadIdx.x] = a;
  __syncthreads();
  if (s == 0 && q < nq) {
    float r = 0.f;
#pragma unroll
    for (int l = 0; l < 16; ++l) r += s_red[l * 16 + col];
    if (q < nw) dw[q] = r;
    else db[q - nw] = r;
  }
}

// ---- float64: one element per thread, plain double fma in the same k order (a yardstick for gradcheck) ------------
__global__ __launch_bounds__(256) void k_cw_forward_f64(const double *__restrict__ src, int c,
                                                       const double *__restrict__ w, const double *__restrict__ bias,
                                                       const int32_t *__restrict__ tbl, int64_t n_tgt, int volume,
                                                       double *__restrict__ dst) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_tgt * c) return;
  const int64_t t = idx / c;
  const int ch = (int)(idx % c);
  double acc = 0.0;
  for (int k = 0; k < volume; ++k) {
    const int32_t s = tbl[(int64_t)k * n_tgt + t];
    if (s < 0) continue;
    acc = fma(w[(int64_t)k * c + ch], src[(int64_t)s * c + ch], acc);
  }
  if (bias) acc += bias[ch];
  dst[idx] = acc;
}

// column q < volume * c: dW[k][ch] = sum over the source rows i (ascending) of x[i][ch] * dy[nbrT[k][i]][ch];
// q >= volume * c: db[ch] = sum over the output rows of dy[t][ch]
__global__ __launch_bounds__(256) void k_cw_wgrad_f64(const double *__restrict__ x, const double *__restrict__ dy,
                                                     int c, const int32_t *__restrict__ tbl_t, int64_t n_in,
                                                     int64_t n_out, int volume, int has_db, double *__restrict__ dw,
                                                     double *__restrict__ db) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nw = (int64_t)volume * c;
  if (q >= nw + (has_db ? c : 0)) return;
  double acc = 0.0;
  if (q < nw) {
    const int64_t k = q / c;
    const int ch = (int)(q % c);
    for (int64_t i = 0; i < n_in; ++i) {
      const int32_t o = tbl_t[k * n_in + i];
      if (o >= 0) acc = fma(x[i * c + ch], dy[(int64_t)o * c + ch], acc);
    }
    dw[q] = acc;
  } else {
    const int ch = (int)(q - nw);
    for (int64_t t = 0; t < n_out; ++t) acc += dy[t * c + ch];
    db[ch] = acc;
  }
}

}  // namespace cw
}  // namespace me

using namespace me;
using namespace me::cw;

namespace {

constexpr int kCwRowsPerChunk = 256;   // chunk size of the backward partials ...
constexpr int kCwMaxChunks = 512;      // ... and their number (the final kernel reads chunks x (volume + 1) x c floats)
constexpr int kCwMaxVolume = 65535;

int64_t cw_chunks(int64_t n_in) {
  const int64_t g = ceil_div(n_in < 1 ? 1 : n_in, kCwRowsPerChunk);
  return g < kCwMaxChunks ? g : kCwMaxChunks;
}

template <typename T>
int cw_launch_forward(const T *src, int c, const float *w, const float *bias, const int32_t *tbl, int64_t n_src,
                      int64_t n_tgt, int volume, T *dst, hipStream_t stream) {
  // 16 bytes of features (4 fp32 / 8 bf16) or 8 bytes of bf16; the weights and the bias are fp32: 16 bytes per piece
  const int v = aligned({w, bias}, 16) ? piece_width<T>(kPieceBf16Half, c, {src, dst}) : 1;
  const dim3 grid = piece_grid(n_tgt, c, v), block(256);
  ME_PIECE_DISPATCH(T, kPieceBf16Half, v, hipLaunchKernelGGL((k_cw_forward<T, V>), grid, block, 0, stream, src, c, w, bias,
                                                            tbl, n_src, n_tgt, volume, dst));
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int cw_forward(const T *src, int32_t c, const float *w, const float *bias, const int32_t *tbl, int64_t n_src,
               int64_t n_tgt, int64_t volume, T *dst, hipStream_t stream) {
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(volume >= 1 && volume <= kCwMaxVolume, "kernel volume must be in [1, 65535]");
  if (n_tgt == 0) return 0;
  return cw_launch_forward<T>(src, c, w, bias, tbl, n_src, n_tgt, (int)volume, dst, stream);
}

template <typename T, int V, int KG>
int cw_backward_v(const T *x, const T *dy, int c, const float *w, const int32_t *tbl_t, int64_t n_in, int64_t n_out,
                  int volume, int need_dx, T *dx, float *dw, float *db, float *part, hipStream_t stream) {
  const int64_t chunks = cw_chunks(n_in);
  const int kgroups = (int)ceil_div(volume, KG);
  const dim3 grid((unsigned)chunks, (unsigned)kgroups), block(256);
  const bool fused = need_dx && kgroups == 1;
  const int has_db = db != nullptr;
  if (fused)
    hipLaunchKernelGGL((k_cw_backward_partial<T, V, KG, true>), grid, block, 0, stream, x, dy, c, w, tbl_t, n_in, n_out,
                       volume, (int)chunks, has_db, dx, part);
  else
    hipLaunchKernelGGL((k_cw_backward_partial<T, V, KG, false>), grid, block, 0, stream, x, dy, c, w, tbl_t, n_in,
                       n_out, volume, (int)chunks, has_db, dx, part);
  ME_LAUNCH_CHECK();
  const int64_t nw = (int64_t)volume * c, ncol = nw + c;
  const int64_t nq = has_db ? ncol : nw;
  hipLaunchKernelGGL(k_cw_backward_final, dim3((unsigned)ceil_div(nq, 16)), dim3(256), 0, stream, part, (int)chunks,
                     ncol, nw, has_db, dw, db);
  ME_LAUNCH_CHECK();
  if (need_dx && !fused && n_in > 0)   // k-groups: dx by the target-stationary pass over nbrT (same order, same bits)
    return cw_launch_forward<T>(dy, c, w, nullptr, tbl_t, n_out, n_in, volume, dx, stream);
  return 0;
}

template <typename T>
int cw_backward(const T *x, const T *dy, int32_t c, const float *w, const int32_t *tbl_t, int64_t n_in, int64_t n_out,
                int64_t volume, int32_t need_dx, T *dx, float *dw, float *db, void *workspace, int64_t workspace_bytes,
                hipStream_t stream) {
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(volume >= 1 && volume <= kCwMaxVolume, "kernel volume must be in [1, 65535]");
  ME_CHECK(!need_dx || dx != nullptr || n_in == 0, "need_dx without a dx buffer");
  ME_CHECK(dw != nullptr, "dweight must be given");
  if (n_in == 0 && n_out == 0) {   // nothing to read: zero gradients, no launch
    ME_HIP(hipMemsetAsync(dw, 0, (size_t)volume * c * sizeof(float), stream));
    if (db) ME_HIP(hipMemsetAsync(db, 0, (size_t)c * sizeof(float), stream));
    return 0;
  }
  ME_CHECK(workspace != nullptr && workspace_bytes >= me_cwconv_backward_workspace_bytes(n_in, volume, c),
           "workspace too small");
  float *part = reinterpret_cast<float *>(workspace);
  // 4-channel pieces (16 bytes of fp32, 8 of bf16) when c and the row starts allow, else one channel; 16 / 32 offsets
  // per k-group: 64 / 32 register partials (32 offsets of 4-channel pieces took 200 - 256 VGPRs, 1 - 2 waves per SIMD)
  const uintptr_t a = 4 * sizeof(T);
  if (c % 4 == 0 && aligned({x, dy, need_dx ? dx : nullptr}, a) && aligned({w}, 16))
    return cw_backward_v<T, 4, 16>(x, dy, c, w, tbl_t, n_in, n_out, (int)volume, need_dx, dx, dw, db, part, stream);
  return cw_backward_v<T, 1, 32>(x, dy, c, w, tbl_t, n_in, n_out, (int)volume, need_dx, dx, dw, db, part, stream);
}

}  // namespace

extern "C" {

int64_t me_cwconv_backward_workspace_bytes(int64_t n_src, int64_t volume, int32_t c) {
  // partial dW | db rows of every chunk: [chunks][volume * c + c] floats
  return align_up(cw_chunks(n_src) * (volume * c + c) * (int64_t)sizeof(float), 256);
}

int me_cwconv_forward_f32(const float *src, int32_t c, const float *weight, const float *bias, const int32_t *tbl,
                          int64_t n_src, int64_t n_tgt, int64_t volume, float *dst, void *stream) {
  return cw_forward<float>(src, c, weight, bias, tbl, n_src, n_tgt, volume, dst, (hipStream_t)stream);
}
int me_cwconv_forward_bf16(const uint16_t *src, int32_t c, const float *weight, const float *bias, const int32_t *tbl,
                           int64_t n_src, int64_t n_tgt, int64_t volume, uint16_t *dst, void *stream) {
  return cw_forward<__bf16>((const __bf16 *)src, c, weight, bias, tbl, n_src, n_tgt, volume, (__bf16 *)dst,
                            (hipStream_t)stream);
}
int me_cwconv_forward_f64(const double *src, int32_t c, const double *weight, const double *bias, const int32_t *tbl,
                          int64_t n_src, int64_t n_tgt, int64_t volume, double *dst, void *stream) {
  (void)n_src;
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(volume >= 1 && volume <= kCwMaxVolume, "kernel volume must be in [1, 65535]");
  if (n_tgt == 0) return 0;
  hipLaunchKernelGGL(k_cw_forward_f64, dim3((unsigned)ceil_div(n_tgt * c, 256)), dim3(256), 0, (hipStream_t)stream,
                     src, c, weight, bias, tbl, n_tgt, (int)volume, dst);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_cwconv_backward_f32(const float *x, const float *dy, int32_t c, const float *weight, const int32_t *tbl_t,
                           int64_t n_src, int64_t n_tgt, int64_t volume, int32_t need_dx, float *dx, float *dweight,
                           float *dbias, void *workspace, int64_t workspace_bytes, void *stream) {
  return cw_backward<float>(x, dy, c, weight, tbl_t, n_src, n_tgt, volume, need_dx, dx, dweight, dbias, workspace,
                            workspace_bytes, (hipStream_t)stream);
}
int me_cwconv_backward_bf16(const uint16_t *x, const uint16_t *dy, int32_t c, const float *weight,
                            const int32_t *tbl_t, int64_t n_src, int64_t n_tgt, int64_t volume, int32_t need_dx,
                            uint16_t *dx, float *dweight, float *dbias, void *workspace, int64_t workspace_bytes,
                            void *stream) {
  return cw_backward<__bf16>((const __bf16 *)x, (const __bf16 *)dy, c, weight, tbl_t, n_src, n_tgt, volume, need_dx,
                             (__bf16 *)dx, dweight, dbias, workspace, workspace_bytes, (hipStream_t)stream);
}
int me_cwconv_backward_f64(const double *x, const double *dy, int32_t c, const double *weight, const int32_t *tbl_t,
                           int64_t n_src, int64_t n_tgt, int64_t volume, int32_t need_dx, double *dx, double *dweight,
                           double *dbias, void *workspace, int64_t workspace_bytes, void *stream_) {
  (void)workspace;
  (void)workspace_bytes;
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(volume >= 1 && volume <= kCwMaxVolume, "kernel volume must be in [1, 65535]");
  ME_CHECK(!need_dx || dx != nullptr || n_src == 0, "need_dx without a dx buffer");
  ME_CHECK(dweight != nullptr, "dweight must be given");
  const int64_t nq = volume * c + (dbias ? c : 0);
  hipLaunchKernelGGL(k_cw_wgrad_f64, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, stream, x, dy, c, tbl_t, n_src,
                     n_tgt, (int)volume, dbias != nullptr, dweight, dbias);
  ME_LAUNCH_CHECK();
  if (need_dx && n_src > 0) {
    hipLaunchKernelGGL(k_cw_forward_f64, dim3((unsigned)ceil_div(n_src * c, 256)), dim3(256), 0, stream, dy, c, weight,
                       (const double *)nullptr, tbl_t, n_src, (int)volume, dx);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_conv_channelwise(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::cw::k_cw_forward<float, 4>));
}
