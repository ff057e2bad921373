// Tensor fields for gfx950 (MI355X): quantisation of continuous coordinates, field -> sparse lookups, the trilinear
// interpolation map, and the one feature-movement kernel every field operator runs on (a weighted CSR gather-sum).
//
// The reference builds its maps with quantize_coordinates_kernel, field_map_kernel and interpolation_kernel
// (src/coordinate_map_gpu.cu:107-145, 1977-2112) followed by a thrust remove_if, and moves every feature through
// cuSPARSE coo_spmm (src/spmm.cu, src/interpolation_gpu.cu).  Here:
//   * the maps probe the library's own open-addressing table (table_find<NCOL>, common.hpp) and compact with a
//     per-point count, the library's scan and an ordered write: entries come out in the reference's order after its
//     stable remove_if, (point, corner) ascending, and the forward row pointer falls out of the scan;
//   * the transpose to rows of another index (interpolation backward, splat, voxel sums) is the library's stable LSD
//     radix sort (coords.hip) plus a binary-search row pointer: stable in entry order, no atomics;
//   * every feature movement is k_csr_gather: y[r] = scale[r] * sum_{e in row r} w_e * x[col_e], row-stationary, sums in
//     entry order (fp32 for fp32 and bf16 features, double for float64), each output row written once (empty rows: 0).
// So every result is bitwise reproducible, as the convolution path is.
#include "piece.hpp"

#include <math.h>

namespace me {
int64_t radix_argsort_workspace_bytes(int64_t n);
int radix_argsort_u32(const uint32_t *keys, int64_t n, int bits, uint32_t *sorted_keys, uint32_t *order, void *ws,
                      int64_t ws_bytes, hipStream_t stream);

namespace field {

constexpr int kMaxD = 7;
struct Strides {
  int32_t s[kMaxD];
};

// voxel corner of column j (1..D): floor(x / s) * s (a division, not a reciprocal product, like the reference)
template <typename F>
__device__ __forceinline__ int32_t quantize_col(F x, int32_t s) {
  return (int32_t)(floor(x / (F)s) * (F)s);
}

// Byte model: n * ncol * (sizeof(F) + 4).
template <typename F, int NCOL>
__global__ __launch_bounds__(256) void k_quantize(const F *__restrict__ x, int64_t n, Strides st,
                                                 int32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i * NCOL] = (int32_t)lrint(x[i * NCOL]);
#pragma unroll
  for (int j = 1; j < NCOL; ++j) out[i * NCOL + j] = quantize_col<F>(x[i * NCOL + j], st.s[j - 1]);
}

// rows[i] = map row of the voxel of point i or -1; flag[i] = hit.  Byte model: n * (ncol * sizeof(F) + 8) plus the
// probes (one 8-byte slot read per probe step, one coordinate row per tag match).
template <typename F, int NCOL>
__global__ __launch_bounds__(256) void k_lookup(const F *__restrict__ x, int64_t n, Strides st,
                                               const uint64_t *__restrict__ table, uint32_t mask,
                                               const int32_t *__restrict__ map_coords, int32_t *__restrict__ rows,
                                               uint32_t *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t key[NCOL];
  key[0] = (int32_t)lrint(x[i * NCOL]);
#pragma unroll
  for (int j = 1; j < NCOL; ++j) key[j] = quantize_col<F>(x[i * NCOL + j], st.s[j - 1]);
  const int32_t r = table_find<NCOL>(table, mask, map_coords, key);
  rows[i] = r;
  flag[i] = r >= 0 ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_lookup_compact(const int32_t *__restrict__ rows, const uint32_t *__restrict__ pos,
                                                       int64_t n, int32_t *__restrict__ sparse_rows,
                                                       int32_t *__restrict__ field_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t r = rows[i];
  if (r >= 0) {
    sparse_rows[pos[i]] = r;
    field_rows[pos[i]] = (int32_t)i;
  }
}

// rows[i] = row of the ORIGIN map (tensor stride 0: coordinates (batch, 0, .., 0)) of point i's batch index lrint(x_0),
// or -1: the row table of global pooling / broadcast over a field.  Byte model: n * (ncol * 4 (one column used) + 4).
template <int NCOL>
__global__ __launch_bounds__(256) void k_origin_rows(const float *__restrict__ x, int64_t n,
                                                    const uint64_t *__restrict__ table, uint32_t mask,
                                                    const int32_t *__restrict__ map_coords, int32_t *__restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t key[NCOL];
  key[0] = (int32_t)lrint(x[i * NCOL]);
#pragma unroll
  for (int j = 1; j < NCOL; ++j) key[j] = 0;
  rows[i] = table_find<NCOL>(table, mask, map_coords, key);
}

// corner n of point x: bit (D - j) of n selects floor(x_j / s_j) * s_j + s_j in column j
template <typename F, int NCOL>
__device__ __forceinline__ void corner(const F (&xf)[NCOL], const Strides &st, int n, int32_t (&c)[NCOL]) {
  c[0] = (int32_t)lrint(xf[0]);
#pragma unroll
  for (int j = 1; j < NCOL; ++j) {
    const int32_t s = st.s[j - 1];
    c[j] = quantize_col<F>(xf[j], s) + (((n >> (NCOL - 1 - j)) & 1) ? s : 0);
  }
}

// Pass 1, one thread per (point, corner): dense[p * 2^D + n] = map row of the corner or -1, and per point the number of
// present corners (the 2^D corner threads of a point are consecutive lanes of one wave: a ballot counts them).
// Byte model: n * (ncol * sizeof(F) * 2^D (cache hits after the first) + 4 * 2^D + 4) plus the probes.
template <typename F, int NCOL>
__global__ __launch_bounds__(256) void k_interp_probe(const F *__restrict__ x, int64_t n, Strides st,
                                                     const uint64_t *__restrict__ table, uint32_t mask,
                                                     const int32_t *__restrict__ map_coords,
                                                     int32_t *__restrict__ dense, uint32_t *__restrict__ count) {
  constexpr int NV = 1 << (NCOL - 1);
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = t < n * NV;
  int32_t r = -1;
  if (valid) {
    const int64_t p = t / NV;
    F xf[NCOL];
#pragma unroll
    for (int j = 0; j < NCOL; ++j) xf[j] = x[p * NCOL + j];
    int32_t c[NCOL];
    corner<F, NCOL>(xf, st, (int)(t % NV), c);
    r = table_find<NCOL>(table, mask, map_coords, c);
    dense[t] = r;
  }
  if constexpr (NV <= 64) {
    const unsigned long long m = __ballot(r >= 0);
    const int lane = lane_id();
    if (valid && (lane % NV) == 0) count[t / NV] = (uint32_t)__popcll((m >> lane) & (~0ull >> (64 - NV)));
  } else {
    // (D >= 7: 128 corners per point) one thread per point counts its own corners after the wave's probes
    (void)count;
  }
}

template <typename F, int NCOL>
__global__ __launch_bounds__(256) void k_interp_count_wide(const int32_t *__restrict__ dense, int64_t n,
                                                          uint32_t *__restrict__ count) {
  constexpr int NV = 1 << (NCOL - 1);
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint32_t k = 0;
  for (int v = 0; v < NV; ++v) k += dense[p * NV + v] >= 0 ? 1u : 0u;
  count[p] = k;
}

// Pass 2, one thread per point: its present corners in corner order at pos[p] ..., weight
// w = prod_{j=1..D} (1 - |x_j - c_j| / s_j) in the coordinate type, j ascending (interpolation_kernel's formula).
// Byte model: n * (ncol * sizeof(F) + 4 * 2^D + 4) + nnz * (8 + sizeof(F)).
template <typename F, int NCOL>
__global__ __launch_bounds__(256) void k_interp_fill(const F *__restrict__ x, int64_t n, Strides st,
                                                    const int32_t *__restrict__ dense,
                                                    const uint32_t *__restrict__ pos, int32_t *__restrict__ in_rows,
                                                    int32_t *__restrict__ out_rows, F *__restrict__ w,
                                                    int32_t *__restrict__ rowptr) {
  constexpr int NV = 1 << (NCOL - 1);
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  F xf[NCOL];
#pragma unroll
  for (int j = 0; j < NCOL; ++j) xf[j] = x[p * NCOL + j];
  uint32_t o = pos[p];
  rowptr[p] = (int32_t)o;
  for (int v = 0; v < NV; ++v) {
    const int32_t r = dense[p * NV + v];
    if (r < 0) continue;
    int32_t c[NCOL];
    corner<F, NCOL>(xf, st, v, c);
    F wt = 1;
#pragma unroll
    for (int j = 1; j < NCOL; ++j) wt *= (F)1 - fabs(xf[j] - (F)c[j]) / (F)st.s[j - 1];
    in_rows[o] = r;
    out_rows[o] = (int32_t)p;
    w[o] = wt;
    ++o;
  }
}

// ---- CSR from COO (stable by entry) ------------------------------------------------------------------------------------
// rowptr[k] = first position of key k in the sorted keys (binary search; rowptr[n_rows] = nnz).
// Byte model: (n_rows + 1) * (4 + log2(nnz) * 4, cache hits).
__global__ __launch_bounds__(256) void k_csr_rowptr(const uint32_t *__restrict__ sorted, int64_t nnz, int64_t n_rows,
                                                   int32_t *__restrict__ rowptr) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_rows) return;
  int64_t lo = 0, hi = nnz;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)sorted[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  rowptr[k] = (int32_t)lo;
}

// cols_out[i] = cols[order[i]] (or order[i]), vals_out[i] = vals[order[i]].  Byte model: nnz * (4 + 4 + 2 * vb).
template <typename W>
__global__ __launch_bounds__(256) void k_csr_permute(const uint32_t *__restrict__ order, int64_t nnz,
                                                    const int32_t *__restrict__ cols, const W *__restrict__ vals,
                                                    int32_t *__restrict__ cols_out, W *__restrict__ vals_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const uint32_t e = order[i];
  cols_out[i] = cols ? cols[e] : (int32_t)e;
  if (vals_out) vals_out[i] = vals[e];
}

// ---- the weighted CSR gather-sum ------------------------------------------------------------------------------------
// A lane owns a (row, V-channel piece): the row's entries are read EB at a time (index and weight loads clamped to the
// row's last entry, so every load is unconditional; the value is masked), then EB feature pieces, then added in entry
// order.  Accumulation in A (fp32 for fp32 / bf16 features, double for float64): fma(w, x, acc), or acc + x without
// weights; scale multiplies the finished sum.  Byte model: e * C * (n_rows + n_distinct_cols) + 8 * nnz
// (e = feature element size; the gathered rows are L2 / MALL hits after their first read).
constexpr int EB = 8;

template <typename T, typename A, int V>
__global__ __launch_bounds__(256) void k_csr_gather(const T *__restrict__ x, int c, const int32_t *__restrict__ rowptr,
                                                   const int32_t *__restrict__ col, const A *__restrict__ w,
                                                   const A *__restrict__ scale, int64_t n_rows, T *__restrict__ y) {
  const int pieces = c / V;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_rows * pieces) return;
  const int64_t r = idx / pieces;
  const int ch = (int)(idx % pieces) * V;
  const int32_t e0 = rowptr[r], e1 = rowptr[r + 1];
  Piece<V, A> acc;
#pragma unroll
  for (int j = 0; j < V; ++j) acc.v[j] = (A)0;
  for (int32_t b0 = e0; b0 < e1; b0 += EB) {
    int32_t s[EB];
    A wt[EB];
#pragma unroll
    for (int b = 0; b < EB; ++b) {
      const int32_t e = min(b0 + b, e1 - 1);
      s[b] = col[e];
      wt[b] = w ? w[e] : (A)1;
    }
    Piece<V, A> xv[EB];
#pragma unroll
    for (int b = 0; b < EB; ++b) xv[b] = load_piece<T, V, A>(x + (int64_t)s[b] * c + ch);
#pragma unroll
    for (int b = 0; b < EB; ++b) {
      if (b0 + b < e1) {
        if (w) {
#pragma unroll
          for (int j = 0; j < V; ++j) acc.v[j] = fma(wt[b], xv[b].v[j], acc.v[j]);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) acc.v[j] += xv[b].v[j];
        }
      }
    }
  }
  if (scale) {
    const A sc = scale[r];
#pragma unroll
    for (int j = 0; j < V; ++j) acc.v[j] *= sc;
  }
  store_piece<T, V, A>(y + r * c + ch, acc);
}

template <typename T, typename A>
int csr_gather(const T *x, int32_t c, const int32_t *rowptr, const int32_t *col, const A *w, const A *scale,
               int64_t n_rows, T *y, hipStream_t stream) {
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(n_rows >= 0, "invalid row count");
  if (n_rows == 0) return 0;
  ME_CHECK(rowptr != nullptr && y != nullptr, "rowptr and y must be given");
  const int v = piece_width<T>(kPieceHalf, c, {x, y});   // (the 8-byte piece: bf16 rows of 20 channels are 40 bytes)
  const dim3 grid = piece_grid(n_rows, c, v), block(256);
  ME_PIECE_DISPATCH(T, kPieceHalf, v, hipLaunchKernelGGL((k_csr_gather<T, A, V>), grid, block, 0, stream, x, c, rowptr, col,
                                                        w, scale, n_rows, y));
  ME_LAUNCH_CHECK();
  return 0;
}

Strides strides_of(const int32_t *ts, int ncol) {
  Strides st;
  for (int j = 0; j < kMaxD; ++j) st.s[j] = (ts != nullptr && j < ncol - 1) ? ts[j] : 1;
  return st;
}

int check_strides(const Strides &st, int ncol) {
  for (int j = 0; j < ncol - 1; ++j) ME_CHECK(st.s[j] > 0, "tensor strides must be positive");
  return 0;
}

template <typename F>
int quantize(const F *x, int64_t n, int32_t ncol, const int32_t *ts, int32_t *out, hipStream_t stream) {
  ME_CHECK(ncol >= 2 && ncol <= 8, "coordinate size (D+1) must be in [2, 8]");
  const Strides st = strides_of(ts, ncol);
  if (int rc = check_strides(st, ncol)) return rc;
  if (n == 0) return 0;
  const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL((k_quantize<F, NCOL>), grid, block, 0, stream, x, n, st, out));
  ME_LAUNCH_CHECK();
  return 0;
}

int64_t lookup_ws(int64_t n) { return 2 * align_up((n > 0 ? n : 1) * 4, 256) + 256 + scan_workspace_bytes(n); }

template <typename F>
int lookup(const F *x, int64_t n, int32_t ncol, const int32_t *ts, const uint64_t *table, int64_t capacity,
           const int32_t *map_coords, int32_t *sparse_rows, int32_t *field_rows, int64_t *n_hit, void *ws,
           int64_t ws_bytes, hipStream_t stream) {
  ME_CHECK(ncol >= 2 && ncol <= 8, "coordinate size (D+1) must be in [2, 8]");
  ME_CHECK(capacity >= 64 && (capacity & (capacity - 1)) == 0, "capacity must be a power of two");
  ME_CHECK(n >= 0 && n < (1ll << 31), "number of points must fit in int32");
  ME_CHECK(ncol != 4 || (uintptr_t)map_coords % 16 == 0, "coordinates with 4 columns must be 16-byte aligned");
  ME_CHECK(n_hit != nullptr, "n_hit must be given");
  const Strides st = strides_of(ts, ncol);
  if (int rc = check_strides(st, ncol)) return rc;
  *n_hit = 0;
  if (n == 0) return 0;
  ME_CHECK(ws != nullptr && ws_bytes >= lookup_ws(n), "workspace too small");
  char *p = reinterpret_cast<char *>(ws);
  const int64_t a = align_up(n * 4, 256);
  int32_t *rows = reinterpret_cast<int32_t *>(p);
  uint32_t *flag = reinterpret_cast<uint32_t *>(p + a);
  uint32_t *total = reinterpret_cast<uint32_t *>(p + 2 * a);
  void *scan_ws = p + 2 * a + 256;
  const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
  const uint32_t mask = (uint32_t)(capacity - 1);
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL((k_lookup<F, NCOL>), grid, block, 0, stream, x, n, st, table, mask,
                                            map_coords, rows, flag));
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(flag, flag, n, total, scan_ws, scan_workspace_bytes(n), stream)) return rc;
  hipLaunchKernelGGL(k_lookup_compact, grid, block, 0, stream, rows, flag, n, sparse_rows, field_rows);
  ME_LAUNCH_CHECK();
  uint32_t h = 0;
  ME_HIP(hipMemcpyAsync(&h, total, 4, hipMemcpyDeviceToHost, stream));
  ME_HIP(hipStreamSynchronize(stream));
  *n_hit = h;
  return 0;
}

int64_t interp_ws(int64_t n, int32_t ncol) {
  const int64_t nv = (int64_t)1 << (ncol - 1);
  const int64_t m = n > 0 ? n : 1;
  return align_up(m * nv * 4, 256) + align_up(m * 4, 256) + 256 + scan_workspace_bytes(m);
}

template <typename F>
int interp_map(const F *x, int64_t n, int32_t ncol, const int32_t *ts, const uint64_t *table, int64_t capacity,
               const int32_t *map_coords, int32_t *in_rows, int32_t *out_rows, F *weights, int32_t *rowptr,
               int64_t *nnz, void *ws, int64_t ws_bytes, hipStream_t stream) {
  ME_CHECK(ncol >= 2 && ncol <= 8, "coordinate size (D+1) must be in [2, 8]");
  ME_CHECK(capacity >= 64 && (capacity & (capacity - 1)) == 0, "capacity must be a power of two");
  ME_CHECK(n >= 0 && (n << (ncol - 1)) < (1ll << 31), "points x corners must fit in int32");
  ME_CHECK(ncol != 4 || (uintptr_t)map_coords % 16 == 0, "coordinates with 4 columns must be 16-byte aligned");
  ME_CHECK(nnz != nullptr && rowptr != nullptr, "nnz and rowptr must be given");
  const Strides st = strides_of(ts, ncol);
  if (int rc = check_strides(st, ncol)) return rc;
  *nnz = 0;
  if (n == 0) {
    ME_HIP(hipMemsetAsync(rowptr, 0, 4, stream));
    return 0;
  }
  ME_CHECK(ws != nullptr && ws_bytes >= interp_ws(n, ncol), "workspace too small");
  const int64_t nv = (int64_t)1 << (ncol - 1);
  char *p = reinterpret_cast<char *>(ws);
  int32_t *dense = reinterpret_cast<int32_t *>(p);
  p += align_up(n * nv * 4, 256);
  uint32_t *count = reinterpret_cast<uint32_t *>(p);
  p += align_up(n * 4, 256);
  uint32_t *total = reinterpret_cast<uint32_t *>(p);
  void *scan_ws = p + 256;
  const uint32_t mask = (uint32_t)(capacity - 1);
  const dim3 grid_t((unsigned)ceil_div(n * nv, 256)), grid_p((unsigned)ceil_div(n, 256)), block(256);
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL((k_interp_probe<F, NCOL>), grid_t, block, 0, stream, x, n, st, table, mask,
                                            map_coords, dense, count));
  ME_LAUNCH_CHECK();
  if (nv > 64) {
    ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL((k_interp_count_wide<F, NCOL>), grid_p, block, 0, stream, dense, n,
                                              count));
    ME_LAUNCH_CHECK();
  }
  if (int rc = exclusive_scan_u32(count, count, n, total, scan_ws, scan_workspace_bytes(n), stream)) return rc;
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL((k_interp_fill<F, NCOL>), grid_p, block, 0, stream, x, n, st, dense, count,
                                            in_rows, out_rows, weights, rowptr));
  ME_LAUNCH_CHECK();
  ME_HIP(hipMemcpyAsync(rowptr + n, total, 4, hipMemcpyDeviceToDevice, stream));
  uint32_t h = 0;
  ME_HIP(hipMemcpyAsync(&h, total, 4, hipMemcpyDeviceToHost, stream));
  ME_HIP(hipStreamSynchronize(stream));
  *nnz = h;
  return 0;
}

}  // namespace field
}  // namespace me

using namespace me;
using namespace me::field;

extern "C" {

int me_field_quantize_f32(const float *x, int64_t n, int32_t ncol, const int32_t *ts, int32_t *out, void *stream) {
  return quantize<float>(x, n, ncol, ts, out, (hipStream_t)stream);
}
int me_field_quantize_f64(const double *x, int64_t n, int32_t ncol, const int32_t *ts, int32_t *out, void *stream) {
  return quantize<double>(x, n, ncol, ts, out, (hipStream_t)stream);
}

int64_t me_field_lookup_workspace_bytes(int64_t n) { return lookup_ws(n); }
int me_field_lookup_f32(const float *x, int64_t n, int32_t ncol, const int32_t *ts, const uint64_t *table,
                        int64_t capacity, const int32_t *map_coords, int32_t *sparse_rows, int32_t *field_rows,
                        int64_t *n_hit, void *ws, int64_t ws_bytes, void *stream) {
  return lookup<float>(x, n, ncol, ts, table, capacity, map_coords, sparse_rows, field_rows, n_hit, ws, ws_bytes,
                       (hipStream_t)stream);
}
int me_field_lookup_f64(const double *x, int64_t n, int32_t ncol, const int32_t *ts, const uint64_t *table,
                        int64_t capacity, const int32_t *map_coords, int32_t *sparse_rows, int32_t *field_rows,
                        int64_t *n_hit, void *ws, int64_t ws_bytes, void *stream) {
  return lookup<double>(x, n, ncol, ts, table, capacity, map_coords, sparse_rows, field_rows, n_hit, ws, ws_bytes,
                        (hipStream_t)stream);
}

int me_field_origin_rows_f32(const float *x, int64_t n, int32_t ncol, const uint64_t *table, int64_t capacity,
                             const int32_t *origin_coords, int32_t *rows, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(ncol >= 2 && ncol <= 8, "coordinate size (D+1) must be in [2, 8]");
  ME_CHECK(capacity >= 64 && (capacity & (capacity - 1)) == 0, "capacity must be a power of two");
  ME_CHECK(n >= 0 && n < (1ll << 31), "number of points must fit in int32");
  ME_CHECK(ncol != 4 || (uintptr_t)origin_coords % 16 == 0, "coordinates with 4 columns must be 16-byte aligned");
  if (n == 0) return 0;
  ME_CHECK(x != nullptr && table != nullptr && origin_coords != nullptr && rows != nullptr, "null pointer");
  const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
  const uint32_t mask = (uint32_t)(capacity - 1);
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL((k_origin_rows<NCOL>), grid, block, 0, stream, x, n, table, mask,
                                            origin_coords, rows));
  ME_LAUNCH_CHECK();
  return 0;
}

int64_t me_field_interp_workspace_bytes(int64_t n, int32_t ncol) {
  if (ncol < 2 || ncol > 8) return -1;
  return interp_ws(n, ncol);
}
int me_field_interp_map_f32(const float *x, int64_t n, int32_t ncol, const int32_t *ts, const uint64_t *table,
                            int64_t capacity, const int32_t *map_coords, int32_t *in_rows, int32_t *out_rows,
                            float *weights, int32_t *rowptr, int64_t *nnz, void *ws, int64_t ws_bytes, void *stream) {
  return interp_map<float>(x, n, ncol, ts, table, capacity, map_coords, in_rows, out_rows, weights, rowptr, nnz, ws,
                           ws_bytes, (hipStream_t)stream);
}
int me_field_interp_map_f64(const double *x, int64_t n, int32_t ncol, const int32_t *ts, const uint64_t *table,
                            int64_t capacity, const int32_t *map_coords, int32_t *in_rows, int32_t *out_rows,
                            double *weights, int32_t *rowptr, int64_t *nnz, void *ws, int64_t ws_bytes, void *stream) {
  return interp_map<double>(x, n, ncol, ts, table, capacity, map_coords, in_rows, out_rows, weights, rowptr, nnz, ws,
                            ws_bytes, (hipStream_t)stream);
}

int64_t me_csr_from_coo_workspace_bytes(int64_t nnz) {
  return 2 * align_up((nnz > 0 ? nnz : 1) * 4, 256) + radix_argsort_workspace_bytes(nnz);
}
int me_csr_from_coo(const int32_t *keys, const int32_t *cols, const void *vals, int32_t val_bytes, int64_t nnz,
                    int64_t n_rows, int32_t *rowptr, int32_t *cols_out, void *vals_out, void *ws, int64_t ws_bytes,
                    void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(nnz >= 0 && nnz < (1ll << 31) && n_rows >= 0 && n_rows < (1ll << 31), "sizes must fit in int32");
  ME_CHECK(val_bytes == 4 || val_bytes == 8 || vals == nullptr, "values must be 4 or 8 bytes");
  ME_CHECK(rowptr != nullptr && cols_out != nullptr, "rowptr and cols_out must be given");
  if (nnz == 0) {   // (an empty vals array has no address: nothing to pair with vals_out)
    ME_HIP(hipMemsetAsync(rowptr, 0, (size_t)(n_rows + 1) * 4, stream));
    return 0;
  }
  ME_CHECK((vals == nullptr) == (vals_out == nullptr), "vals and vals_out go together");
  ME_CHECK(ws != nullptr && ws_bytes >= me_csr_from_coo_workspace_bytes(nnz), "workspace too small");
  char *p = reinterpret_cast<char *>(ws);
  const int64_t a = align_up(nnz * 4, 256);
  uint32_t *sorted = reinterpret_cast<uint32_t *>(p);
  uint32_t *order = reinterpret_cast<uint32_t *>(p + a);
  int bits = 0;
  while (bits < 32 && (1ll << bits) < n_rows) ++bits;
  if (int rc = radix_argsort_u32(reinterpret_cast<const uint32_t *>(keys), nnz, bits, sorted, order, p + 2 * a,
                                 radix_argsort_workspace_bytes(nnz), stream))
    return rc;
  hipLaunchKernelGGL(k_csr_rowptr, dim3((unsigned)ceil_div(n_rows + 1, 256)), dim3(256), 0, stream, sorted, nnz, n_rows,
                     rowptr);
  ME_LAUNCH_CHECK();
  const dim3 grid((unsigned)ceil_div(nnz, 256)), block(256);
  if (val_bytes == 8)
    hipLaunchKernelGGL(k_csr_permute<uint64_t>, grid, block, 0, stream, order, nnz, cols,
                       reinterpret_cast<const uint64_t *>(vals), cols_out, reinterpret_cast<uint64_t *>(vals_out));
  else
    hipLaunchKernelGGL(k_csr_permute<uint32_t>, grid, block, 0, stream, order, nnz, cols,
                       reinterpret_cast<const uint32_t *>(vals), cols_out, reinterpret_cast<uint32_t *>(vals_out));
  ME_LAUNCH_CHECK();
  return 0;
}

int me_csr_gather_f32(const float *x, int32_t c, const int32_t *rowptr, const int32_t *col, const float *w,
                      const float *scale, int64_t n_rows, float *y, void *stream) {
  return csr_gather<float, float>(x, c, rowptr, col, w, scale, n_rows, y, (hipStream_t)stream);
}
int me_csr_gather_bf16(const uint16_t *x, int32_t c, const int32_t *rowptr, const int32_t *col, const float *w,
                       const float *scale, int64_t n_rows, uint16_t *y, void *stream) {
  return csr_gather<__bf16, float>((const __bf16 *)x, c, rowptr, col, w, scale, n_rows, (__bf16 *)y,
                                   (hipStream_t)stream);
}
int me_csr_gather_f64(const double *x, int32_t c, const int32_t *rowptr, const int32_t *col, const double *w,
                      const double *scale, int64_t n_rows, double *y, void *stream) {
  return csr_gather<double, double>(x, c, rowptr, col, w, scale, n_rows, y, (hipStream_t)stream);
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_field(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::field::k_csr_rowptr));
}
