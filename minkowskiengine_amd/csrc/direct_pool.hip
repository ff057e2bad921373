// Direct max pooling for gfx950 (MI355X): a segmented max with argmax over an arbitrary (in_map, out_map) pair list, the
// operator behind MinkowskiDirectMaxPoolingFunction (reference: src/direct_max_pool.cpp, src/pooling_max_kernel.cu:55-234).
//
// The reference sorts the caller's maps in place with thrust::sort_by_key, reduces by key for the row starts, fills the
// mask with a separate launch and then runs one thread per (output row, channel) with scalar loads.  Here:
//   * one pass over the maps validates them (range, order when is_sorted) and narrows them to int32 copies: the caller's
//     tensors are never written;
//   * the entries are grouped by output row with the library's stable LSD radix sort (coords.hip) and a binary-search
//     row pointer, the CsrFromCoo pieces of field.hip; is_sorted skips the sort;
//   * k_direct_max is shaped like k_csr_gather: a lane owns an (output row, 16-byte piece), reads the row's indices 8 at
//     a time (clamped to the row's last entry, masked), keeps a running max and its source row per channel in registers
//     and writes the row and its mask once; rows without entries get zeros and the "no source" marker in the same pass;
//   * the comparison is the reference's `max < cur` from the row's first entry, entries in map order (the sort is
//     stable): among equal values the first entry wins;
//   * the backward groups the mask itself: the flat winner indices are sorted (stable, so ascending output row), the head
//     of every run of equal indices sums its run in that order and writes one element.  No floating-point atomics: the
//     gradient is bitwise reproducible, also where one input element wins in several output rows.
#include "piece.hpp"

#include <limits>

namespace me {
int64_t radix_argsort_workspace_bytes(int64_t n);
int radix_argsort_u32(const uint32_t *keys, int64_t n, int bits, uint32_t *sorted_keys, uint32_t *order, void *ws,
                      int64_t ws_bytes, hipStream_t stream);

namespace dpool {

constexpr int EB = 8;   // entries in flight per lane, as k_csr_gather

// One pass over the maps: range check, order check (is_sorted), int32 copies.  flag bits: 1 in_map out of range,
// 2 out_map out of range, 4 out_map not ascending.  Byte model: nmap * 2 * (sizeof(I) + 4).
template <typename I>
__global__ __launch_bounds__(256) void k_prepare(const I *__restrict__ in_map, const I *__restrict__ out_map, int64_t nmap,
                                                int64_t in_nrows, int64_t out_nrows, int check_sorted,
                                                uint32_t *__restrict__ keys, int32_t *__restrict__ in32,
                                                uint32_t *__restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nmap) return;
  const int64_t i = (int64_t)in_map[e], o = (int64_t)out_map[e];
  uint32_t bad = 0;
  if (i < 0 || i >= in_nrows) bad |= 1u;
  if (o < 0 || o >= out_nrows) bad |= 2u;
  if (check_sorted && e > 0 && (int64_t)out_map[e - 1] > o) bad |= 4u;
  if (bad) atomicOr(flag, bad);
  keys[e] = (uint32_t)o;
  in32[e] = (int32_t)i;
}

// rowptr[k] = first position of key k in the ascending keys (rowptr[n_rows] = nnz), as k_csr_rowptr of field.hip
__global__ __launch_bounds__(256) void k_rowptr(const uint32_t *__restrict__ sorted, int64_t nnz, int64_t n_rows,
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

__global__ __launch_bounds__(256) void k_permute(const uint32_t *__restrict__ order, int64_t nnz,
                                                const int32_t *__restrict__ vals, int32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  out[i] = vals[order[i]];
}

// A lane owns (output row, V channels).  Values are compared in A (fp32 for bf16: the conversion is exact, so the stored
// winner has its own bits).  Byte model: e * C * (n_rows + n_distinct_in_rows) + sizeof(I) * C * n_rows + 4 * nnz.
template <typename T, typename A, typename I, int V>
__global__ __launch_bounds__(256) void k_direct_max(const T *__restrict__ x, int c, const int32_t *__restrict__ rowptr,
                                                   const int32_t *__restrict__ col, int64_t n_rows, T *__restrict__ y,
                                                   I *__restrict__ mask) {
  const int pieces = c / V;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_rows * pieces) return;
  const int64_t r = idx / pieces;
  const int ch = (int)(idx % pieces) * V;
  const int32_t e0 = rowptr[r], e1 = rowptr[r + 1];
  Piece<V, T> best;
  Piece<V, I> arg;
  if (e0 >= e1) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      best.v[j] = (T)0;
      arg.v[j] = std::numeric_limits<I>::max();
    }
  } else {
    int32_t src[V];
    {
      const int32_t s0 = col[e0];
      best = load_piece<T, V, T>(x + (int64_t)s0 * c + ch);
#pragma unroll
      for (int j = 0; j < V; ++j) src[j] = s0;
    }
    for (int32_t b0 = e0; b0 < e1; b0 += EB) {
      int32_t s[EB];
#pragma unroll
      for (int b = 0; b < EB; ++b) s[b] = col[min(b0 + b, e1 - 1)];
      Piece<V, T> xv[EB];
#pragma unroll
      for (int b = 0; b < EB; ++b) xv[b] = load_piece<T, V, T>(x + (int64_t)s[b] * c + ch);
#pragma unroll
      for (int b = 0; b < EB; ++b) {
        if (b0 + b < e1) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            if ((A)best.v[j] < (A)xv[b].v[j]) {
              best.v[j] = xv[b].v[j];
              src[j] = s[b];
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) arg.v[j] = (I)((int64_t)src[j] * c + ch + j);
  }
  store_piece<T, V, T>(y + r * c + ch, best);
  store_piece<I, V, I>(mask + r * c + ch, arg);
}

inline int bits_for(int64_t n) {
  int bits = 0;
  while (bits < 32 && (1ll << bits) < n) ++bits;
  return bits;
}

struct FwdWs {
  uint32_t *flag, *keys, *sorted, *order;
  int32_t *in32, *cols, *rowptr;
  void *radix;
};
inline int64_t fwd_ws_bytes(int64_t nmap, int64_t out_nrows) {
  const int64_t a = align_up((nmap > 0 ? nmap : 1) * 4, 256);
  return 256 + 5 * a + align_up((out_nrows + 1) * 4, 256) + radix_argsort_workspace_bytes(nmap);
}
inline FwdWs fwd_ws(void *ws, int64_t nmap, int64_t out_nrows) {
  const int64_t a = align_up((nmap > 0 ? nmap : 1) * 4, 256);
  char *p = reinterpret_cast<char *>(ws);
  FwdWs w;
  w.flag = reinterpret_cast<uint32_t *>(p);
  w.keys = reinterpret_cast<uint32_t *>(p + 256);
  w.in32 = reinterpret_cast<int32_t *>(p + 256 + a);
  w.sorted = reinterpret_cast<uint32_t *>(p + 256 + 2 * a);
  w.order = reinterpret_cast<uint32_t *>(p + 256 + 3 * a);
  w.cols = reinterpret_cast<int32_t *>(p + 256 + 4 * a);
  w.rowptr = reinterpret_cast<int32_t *>(p + 256 + 5 * a);
  w.radix = p + 256 + 5 * a + align_up((out_nrows + 1) * 4, 256);
  return w;
}

template <typename T, typename A, typename I>
int launch_max(const T *x, int32_t c, const int32_t *rowptr, const int32_t *col, int64_t n_rows, T *y, I *mask,
               hipStream_t stream) {
  // the mask piece has the channel count of the feature piece: V * sizeof(I) bytes, aligned to its size
  int al = common_alignment({x, y});
  while (al >= 8 && !aligned({mask}, al / sizeof(T) * sizeof(I))) al /= 2;
  const int v = piece_width((int)sizeof(T), c, al, kPieceHalf);
  const dim3 grid = piece_grid(n_rows, c, v), block(256);
  ME_PIECE_DISPATCH(T, kPieceHalf, v, hipLaunchKernelGGL((k_direct_max<T, A, I, V>), grid, block, 0, stream, x, c, rowptr,
                                                        col, n_rows, y, mask));
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, typename A, typename I>
int forward_t(const T *x, int32_t c, const I *in_map, const I *out_map, int64_t nmap, int64_t in_nrows,
              int64_t out_nrows, int is_sorted, T *y, I *mask, void *ws, int64_t ws_bytes, hipStream_t stream) {
  if (out_nrows == 0) return 0;
  const FwdWs w = fwd_ws(ws, nmap, out_nrows);
  const int32_t *cols = w.in32;
  if (nmap > 0) {
    const dim3 grid((unsigned)ceil_div(nmap, 256)), block(256);
    ME_HIP(hipMemsetAsync(w.flag, 0, 4, stream));
    hipLaunchKernelGGL((k_prepare<I>), grid, block, 0, stream, in_map, out_map, nmap, in_nrows, out_nrows,
                       is_sorted ? 1 : 0, w.keys, w.in32, w.flag);
    ME_LAUNCH_CHECK();
    uint32_t bad = 0;
    ME_HIP(hipMemcpyAsync(&bad, w.flag, 4, hipMemcpyDeviceToHost, stream));
    ME_HIP(hipStreamSynchronize(stream));
    ME_CHECK((bad & 1u) == 0, "in_map holds a value outside [0, in_nrows)");
    ME_CHECK((bad & 2u) == 0,
             "out_map holds a value outside [0, out_nrows): Invalid number of out nrows (more output rows than out_nrows)");
    ME_CHECK((bad & 4u) == 0, "is_sorted was given but out_map is not ascending");
    const uint32_t *sorted = w.keys;
    if (!is_sorted) {
      if (int rc = radix_argsort_u32(w.keys, nmap, bits_for(out_nrows), w.sorted, w.order, w.radix,
                                     radix_argsort_workspace_bytes(nmap), stream))
        return rc;
      hipLaunchKernelGGL(k_permute, grid, block, 0, stream, w.order, nmap, w.in32, w.cols);
      ME_LAUNCH_CHECK();
      sorted = w.sorted;
      cols = w.cols;
    }
    hipLaunchKernelGGL(k_rowptr, dim3((unsigned)ceil_div(out_nrows + 1, 256)), dim3(256), 0, stream, sorted, nmap,
                       out_nrows, w.rowptr);
    ME_LAUNCH_CHECK();
  } else {
    ME_HIP(hipMemsetAsync(w.rowptr, 0, (size_t)(out_nrows + 1) * 4, stream));
  }
  return launch_max<T, A, I>(x, c, w.rowptr, cols, out_nrows, y, mask, stream);
}

template <typename T, typename A>
int forward(const T *x, int32_t c, const void *in_map, const void *out_map, int32_t index_bytes, int64_t nmap,
            int64_t in_nrows, int64_t out_nrows, int32_t is_sorted, T *y, void *mask, void *ws, int64_t ws_bytes,
            hipStream_t stream) {
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(index_bytes == 4 || index_bytes == 8, "maps must be int32 or int64");
  ME_CHECK(nmap >= 0 && nmap < (1ll << 31) && in_nrows >= 0 && in_nrows < (1ll << 31) && out_nrows >= 0 &&
               out_nrows < (1ll << 31),
           "sizes must fit in int32");
  ME_CHECK(index_bytes == 8 || in_nrows * c < (1ll << 31), "in_nrows * C must fit the int32 mask: use int64 maps");
  ME_CHECK(nmap == 0 || (in_map != nullptr && out_map != nullptr), "in_map and out_map must be given");
  ME_CHECK(out_nrows == 0 || (y != nullptr && mask != nullptr), "out_feat and max_index must be given");
  ME_CHECK(out_nrows == 0 || nmap == 0 || x != nullptr, "in_feat must be given");
  ME_CHECK(out_nrows == 0 || (ws != nullptr && ws_bytes >= fwd_ws_bytes(nmap, out_nrows)), "workspace too small");
  if (index_bytes == 8)
    return forward_t<T, A, int64_t>(x, c, (const int64_t *)in_map, (const int64_t *)out_map, nmap, in_nrows, out_nrows,
                                    is_sorted, y, (int64_t *)mask, ws, ws_bytes, stream);
  return forward_t<T, A, int32_t>(x, c, (const int32_t *)in_map, (const int32_t *)out_map, nmap, in_nrows, out_nrows,
                                  is_sorted, y, (int32_t *)mask, ws, ws_bytes, stream);
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// keys[i] = flat winner index of mask element i, or `none` (= in_nrows * C) for the marker and anything out of range
template <typename I>
__global__ __launch_bounds__(256) void k_mask_keys(const I *__restrict__ mask, int64_t n, int64_t none,
                                                  uint32_t *__restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t m = (int64_t)mask[i];
  keys[i] = (uint32_t)((m >= 0 && m < none) ? m : none);
}

// The head of every run of equal keys sums the run in sorted (= ascending mask element) order and writes one element
// of grad_in (zeroed before).  Byte model: n * (8 + 2 * e) (the gradient loads are gathers of single elements).
template <typename T, typename A>
__global__ __launch_bounds__(256) void k_segment_sum(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ order,
                                                    int64_t n, uint32_t none, const T *__restrict__ grad_out,
                                                    T *__restrict__ grad_in) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = sorted[i];
  if (k >= none || (i > 0 && sorted[i - 1] == k)) return;
  A acc = (A)grad_out[order[i]];
  for (int64_t j = i + 1; j < n && sorted[j] == k; ++j) acc += (A)grad_out[order[j]];
  grad_in[k] = (T)acc;
}

inline int64_t bwd_ws_bytes(int64_t n) {
  return 3 * align_up((n > 0 ? n : 1) * 4, 256) + radix_argsort_workspace_bytes(n);
}

template <typename T, typename A>
int backward(const T *grad_out, const void *mask, int32_t index_bytes, int64_t out_nrows, int32_t c, int64_t in_nrows,
             T *grad_in, void *ws, int64_t ws_bytes, hipStream_t stream) {
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(index_bytes == 4 || index_bytes == 8, "max_index must be int32 or int64");
  ME_CHECK(out_nrows >= 0 && in_nrows >= 0, "invalid row count");
  const int64_t n = out_nrows * c, none = in_nrows * c;
  ME_CHECK(n < (1ll << 31), "out_nrows * C must fit in int32");
  ME_CHECK(none < (1ll << 32) - 1, "in_nrows * C must fit in uint32");
  if (none == 0) return 0;
  ME_CHECK(grad_in != nullptr, "grad_in must be given");
  ME_HIP(hipMemsetAsync(grad_in, 0, (size_t)none * sizeof(T), stream));
  if (n == 0) return 0;
  ME_CHECK(grad_out != nullptr && mask != nullptr, "grad_out and max_index must be given");
  ME_CHECK(ws != nullptr && ws_bytes >= bwd_ws_bytes(n), "workspace too small");
  char *p = reinterpret_cast<char *>(ws);
  const int64_t a = align_up(n * 4, 256);
  uint32_t *keys = reinterpret_cast<uint32_t *>(p), *sorted = reinterpret_cast<uint32_t *>(p + a),
           *order = reinterpret_cast<uint32_t *>(p + 2 * a);
  const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
  if (index_bytes == 8)
    hipLaunchKernelGGL((k_mask_keys<int64_t>), grid, block, 0, stream, (const int64_t *)mask, n, none, keys);
  else
    hipLaunchKernelGGL((k_mask_keys<int32_t>), grid, block, 0, stream, (const int32_t *)mask, n, none, keys);
  ME_LAUNCH_CHECK();
  if (int rc = radix_argsort_u32(keys, n, bits_for(none + 1), sorted, order, p + 3 * a, radix_argsort_workspace_bytes(n),
                                 stream))
    return rc;
  hipLaunchKernelGGL((k_segment_sum<T, A>), grid, block, 0, stream, sorted, order, n, (uint32_t)none, grad_out, grad_in);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // namespace dpool
}  // namespace me

using namespace me;
using namespace me::dpool;

extern "C" {

int64_t me_direct_max_pool_workspace_bytes(int64_t nmap, int64_t out_nrows) {
  if (nmap < 0 || out_nrows < 0) return -1;
  return fwd_ws_bytes(nmap, out_nrows);
}
int me_direct_max_pool_f32(const float *in_feat, int32_t c, const void *in_map, const void *out_map, int32_t index_bytes,
                           int64_t nmap, int64_t in_nrows, int64_t out_nrows, int32_t is_sorted, float *out_feat,
                           void *max_index, void *ws, int64_t ws_bytes, void *stream) {
  return forward<float, float>(in_feat, c, in_map, out_map, index_bytes, nmap, in_nrows, out_nrows, is_sorted, out_feat,
                               max_index, ws, ws_bytes, (hipStream_t)stream);
}
int me_direct_max_pool_bf16(const uint16_t *in_feat, int32_t c, const void *in_map, const void *out_map,
                            int32_t index_bytes, int64_t nmap, int64_t in_nrows, int64_t out_nrows, int32_t is_sorted,
                            uint16_t *out_feat, void *max_index, void *ws, int64_t ws_bytes, void *stream) {
  return forward<__bf16, float>((const __bf16 *)in_feat, c, in_map, out_map, index_bytes, nmap, in_nrows, out_nrows,
                                is_sorted, (__bf16 *)out_feat, max_index, ws, ws_bytes, (hipStream_t)stream);
}
int me_direct_max_pool_f64(const double *in_feat, int32_t c, const void *in_map, const void *out_map, int32_t index_bytes,
                           int64_t nmap, int64_t in_nrows, int64_t out_nrows, int32_t is_sorted, double *out_feat,
                           void *max_index, void *ws, int64_t ws_bytes, void *stream) {
  return forward<double, double>(in_feat, c, in_map, out_map, index_bytes, nmap, in_nrows, out_nrows, is_sorted,
                                 out_feat, max_index, ws, ws_bytes, (hipStream_t)stream);
}

int64_t me_direct_max_pool_backward_workspace_bytes(int64_t out_nrows, int32_t c) {
  if (out_nrows < 0 || c <= 0) return -1;
  return bwd_ws_bytes(out_nrows * c);
}
int me_direct_max_pool_backward_f32(const float *grad_out, const void *max_index, int32_t index_bytes, int64_t out_nrows,
                                    int32_t c, int64_t in_nrows, float *grad_in, void *ws, int64_t ws_bytes,
                                    void *stream) {
  return backward<float, float>(grad_out, max_index, index_bytes, out_nrows, c, in_nrows, grad_in, ws, ws_bytes,
                                (hipStream_t)stream);
}
int me_direct_max_pool_backward_bf16(const uint16_t *grad_out, const void *max_index, int32_t index_bytes,
                                     int64_t out_nrows, int32_t c, int64_t in_nrows, uint16_t *grad_in, void *ws,
                                     int64_t ws_bytes, void *stream) {
  return backward<__bf16, float>((const __bf16 *)grad_out, max_index, index_bytes, out_nrows, c, in_nrows,
                                 (__bf16 *)grad_in, ws, ws_bytes, (hipStream_t)stream);
}
int me_direct_max_pool_backward_f64(const double *grad_out, const void *max_index, int32_t index_bytes, int64_t out_nrows,
                                    int32_t c, int64_t in_nrows, double *grad_in, void *ws, int64_t ws_bytes,
                                    void *stream) {
  return backward<double, double>(grad_out, max_index, index_bytes, out_nrows, c, in_nrows, grad_in, ws, ws_bytes,
                                  (hipStream_t)stream);
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_direct_pool(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::dpool::k_rowptr));
}
