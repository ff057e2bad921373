// Serialized patch attention for gfx950 (MI355X): the row lists of MinkowskiSerializedSelfAttention.  The voxels of every
// instance are ordered along a space-filling curve, the sequence is cut into patches of at most P rows, and the attention
// kernels of attention.hip attend inside every patch: the patches are the segments of their generic row lists (seg_ptr,
// seg_rows), found through a block table instead of a walk over seg_ptr (me_attn_forward_tab / me_attn_backward_tab).
//
//   k_serial_keys   key = (batch << D depth) | code(x),  x_a = (coords[i, 1 + a] - bbox_min[a]) / tensor_stride[a] < 2^depth
//                     z        bit l of axis a at code bit l D + (D - 1 - a): axis 0 is the most significant of a level
//                     hilbert  Skilling's AxesToTranspose ("Programming the Hilbert curve", AIP Conf. Proc. 707, 2004) on
//                              x with `depth` bits, the transposed axes interleaved by the same rule
//                     *_trans  the same codes with the spatial axes 0 and 1 exchanged beforehand (D >= 2)
//   sort            the library's stable LSD radix sort (coords.hip) over the key bytes that can differ
//   k_inst_bounds / k_inst_start / k_inst_patches / k_row_patch
//                   the instances are the runs of equal batch bits of the sorted keys; an instance of n_b rows has
//                   m_b = ceil(n_b / P) patches and the row of serial rank r goes to patch floor(r m_b / n_b) (64-bit), so the
//                   patch sizes differ by at most one, none exceeds P and no row is borrowed or shared.
//                   row_patch[row] = patch_base[b] + that, patch_base the exclusive scan of m_b in ascending batch order
//   me_csr_from_coo(row_patch) -> seg_ptr [S + 1], seg_rows [n]: rows ascending inside a patch, the fixed summation order
//   k_seg_blocks / k_blk_tab
//                   the block table of the S segments (attn_block.hpp)
// S = ceil(n / P) + n_batch is an upper bound of the patch count that the host knows without a read-back; surplus segments
// are empty.  Everything runs on the caller's stream with no synchronisation.  Nothing here knows that the segments came
// from a curve: any per-row segment id (a window partition, say) gives lists and a table the same way from step
// me_csr_from_coo on.
#include "attn_block.hpp"
#include "common.hpp"

namespace me {

int64_t radix_argsort_u64_workspace_bytes(int64_t n);
int radix_argsort_u64(uint64_t *keys, uint64_t *keys_tmp, int64_t n, const int *shifts, int np, uint32_t *order,
                      uint64_t **sorted_keys, void *ws, int64_t ws_bytes, hipStream_t stream);

struct SerialGeom {
  int32_t bbox_min[ME_MAX_DIM];
  int32_t stride[ME_MAX_DIM];
};

static int bits_of(uint64_t x) {
  int b = 0;
  while (x) { ++b; x >>= 1; }
  return b;
}

template <int NCOL>
__global__ __launch_bounds__(256) void k_serial_keys(const int32_t *__restrict__ coords, int64_t n, SerialGeom g, int depth,
                                                    int order, uint64_t *__restrict__ keys) {
  constexpr int D = NCOL - 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t *c = coords + i * NCOL;
  uint32_t x[D];
  // the difference in uint32: exact modulo 2^32, so exact for every extent an int32 map can have (an int32 difference
  // wraps from an extent of 2^31 on, and the signed quotient is then wrong for a stride that is no power of two)
#pragma unroll
  for (int a = 0; a < D; ++a) x[a] = ((uint32_t)c[1 + a] - (uint32_t)g.bbox_min[a]) / (uint32_t)g.stride[a];
  if constexpr (D >= 2) {
    if (order & 1) { const uint32_t t = x[0]; x[0] = x[1]; x[1] = t; }
  }
  if ((order & 2) && depth > 0) {   // AxesToTranspose
    const uint32_t M = 1u << (depth - 1);
    for (uint32_t Q = M; Q > 1; Q >>= 1) {
      const uint32_t P = Q - 1;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        if (x[a] & Q) {
          x[0] ^= P;
        } else {
          const uint32_t t = (x[0] ^ x[a]) & P;
          x[0] ^= t;
          x[a] ^= t;
        }
      }
    }
#pragma unroll
    for (int a = 1; a < D; ++a) x[a] ^= x[a - 1];
    uint32_t t = 0;
    for (uint32_t Q = M; Q > 1; Q >>= 1)
      if (x[D - 1] & Q) t ^= Q - 1;
#pragma unroll
    for (int a = 0; a < D; ++a) x[a] ^= t;
  }
  uint64_t code = 0;
  for (int l = 0; l < depth; ++l) {
#pragma unroll
    for (int a = 0; a < D; ++a) code |= (uint64_t)((x[a] >> l) & 1u) << (l * D + (D - 1 - a));
  }
  keys[i] = ((uint64_t)(uint32_t)c[0] << (D * depth)) | code;
}

// bound[i] = 1 where sorted positions i and i + 1 belong to different instances: its exclusive scan is the instance of i
__global__ __launch_bounds__(256) void k_inst_bounds(const uint64_t *__restrict__ sk, int64_t n, int shift,
                                                    uint32_t *__restrict__ bound) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bound[i] = (i + 1 < n && (sk[i + 1] >> shift) != (sk[i] >> shift)) ? 1u : 0u;
}

// inst_start [n_batch + 1]: the first sorted position of every instance; n for the instances that do not exist
__global__ __launch_bounds__(256) void k_inst_start(const uint32_t *__restrict__ inst_id, int64_t n, int n_batch,
                                                   uint32_t *__restrict__ inst_start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint32_t b = inst_id[i];
    if ((i == 0 || inst_id[i - 1] != b) && b < (uint32_t)n_batch) inst_start[b] = (uint32_t)i;
  }
  if (i <= n_batch && (uint32_t)i > inst_id[n - 1]) inst_start[i] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void k_inst_patches(const uint32_t *__restrict__ inst_start, int n_batch, int64_t patch,
                                                     uint32_t *__restrict__ inst_m) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_batch) return;
  const int64_t nb = (int64_t)inst_start[b + 1] - (int64_t)inst_start[b];
  inst_m[b] = (uint32_t)((nb + patch - 1) / patch);
}

__global__ __launch_bounds__(256) void k_row_patch(const uint32_t *__restrict__ order, const uint32_t *__restrict__ inst_id,
                                                  const uint32_t *__restrict__ inst_start,
                                                  const uint32_t *__restrict__ patch_base, int64_t n, int n_batch,
                                                  int64_t patch, int64_t n_seg, int32_t *__restrict__ row_patch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = min(inst_id[i], (uint32_t)(n_batch - 1));   // (more instances than n_batch: a caller's error; no stray write)
  const int64_t s0 = inst_start[b], nb = (int64_t)inst_start[b + 1] - s0, r = i - s0;
  const int64_t mb = (nb + patch - 1) / patch;
  int64_t p = (int64_t)patch_base[b] + (nb > 0 ? (int64_t)(((uint64_t)r * (uint64_t)mb) / (uint64_t)nb) : 0);
  p = p < 0 ? 0 : (p > n_seg - 1 ? n_seg - 1 : p);
  row_patch[order[i]] = (int32_t)p;
}

__global__ __launch_bounds__(256) void k_seg_blocks(const int32_t *__restrict__ seg_ptr, int64_t n_seg,
                                                   uint32_t *__restrict__ seg_nblk) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  seg_nblk[s] = (uint32_t)((seg_ptr[s + 1] - seg_ptr[s] + kAttnBlock - 1) / kAttnBlock);
}

__global__ __launch_bounds__(256) void k_blk_tab(const int32_t *__restrict__ seg_ptr, const uint32_t *__restrict__ blk_base,
                                                int64_t n_seg, int64_t n_entries, int32_t *__restrict__ tab) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  const int len = seg_ptr[s + 1] - seg_ptr[s];
  int64_t e = blk_base[s];
  for (int t0 = 0; t0 < len && e < n_entries; t0 += kAttnBlock, ++e) {
    tab[2 * e] = (int32_t)s;
    tab[2 * e + 1] = t0;
  }
}

static int64_t serial_n_seg(int64_t n, int64_t n_batch, int64_t patch) { return ceil_div(n, patch) + n_batch; }

struct SerialWs {
  uint64_t *keys, *keys_tmp;
  uint32_t *order, *inst_id, *inst_start, *inst_m, *seg_nblk, *total;
  void *scan, *sort, *csr;
  int64_t scan_bytes, sort_bytes, csr_bytes, bytes;
};
static SerialWs serial_ws(void *base, int64_t n, int64_t n_batch, int64_t patch) {
  const int64_t m = n < 1 ? 1 : n, n_seg = serial_n_seg(m, n_batch, patch);
  const int64_t scan_n = m > n_seg ? m : n_seg;
  char *p = reinterpret_cast<char *>(base);
  int64_t o = 0;
  auto take = [&](int64_t bytes) { char *q = p + o; o += align_up(bytes, 256); return q; };
  SerialWs w;
  w.keys = reinterpret_cast<uint64_t *>(take(m * 8));
  w.keys_tmp = reinterpret_cast<uint64_t *>(take(m * 8));
  w.order = reinterpret_cast<uint32_t *>(take(m * 4));
  w.inst_id = reinterpret_cast<uint32_t *>(take(m * 4));
  w.inst_start = reinterpret_cast<uint32_t *>(take((n_batch + 1) * 4));
  w.inst_m = reinterpret_cast<uint32_t *>(take((n_batch + 1) * 4));
  w.seg_nblk = reinterpret_cast<uint32_t *>(take(n_seg * 4));
  w.total = reinterpret_cast<uint32_t *>(take(256));
  w.scan_bytes = scan_workspace_bytes(scan_n);
  w.scan = take(w.scan_bytes);
  w.sort_bytes = radix_argsort_u64_workspace_bytes(m);
  w.sort = take(w.sort_bytes);
  w.csr_bytes = me_csr_from_coo_workspace_bytes(m);
  w.csr = take(w.csr_bytes);
  w.bytes = o;
  return w;
}

static int serial_keys(const int32_t *coords, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                       const int32_t *bbox_min, int32_t depth, int32_t order, uint64_t *keys, hipStream_t stream) {
  ME_CHECK(ncol >= 2 && ncol <= ME_MAX_DIM + 1, "invalid coordinate size");
  ME_CHECK(n >= 0 && n < (1ll << 31), "number of rows must fit in int32");
  ME_CHECK(order >= 0 && order <= 3, "order must be 0 (z), 1 (z_trans), 2 (hilbert) or 3 (hilbert_trans)");
  ME_CHECK(tensor_stride != nullptr && bbox_min != nullptr, "tensor_stride and bbox_min must be given");
  ME_CHECK(depth >= 0 && depth <= 31 && (ncol - 1) * depth <= 63, "the serialisation code must fit in 63 bits");
  SerialGeom g{};
  for (int a = 0; a < ncol - 1; ++a) {
    ME_CHECK(tensor_stride[a] > 0, "the tensor stride must be positive");
    g.bbox_min[a] = bbox_min[a];
    g.stride[a] = tensor_stride[a];
  }
  if (n == 0) return 0;
  ME_CHECK(coords != nullptr && keys != nullptr, "null pointer");
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL(k_serial_keys<NCOL>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, stream,
                                            coords, n, g, depth, order, keys));
  ME_LAUNCH_CHECK();
  return 0;
}

}  // namespace me

using namespace me;

extern "C" {

int me_coords_serial_keys(const int32_t *coords, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                          const int32_t *bbox_min, int32_t depth, int32_t order, uint64_t *keys, void *stream) {
  return serial_keys(coords, n, ncol, tensor_stride, bbox_min, depth, order, keys, (hipStream_t)stream);
}

int64_t me_attn_patch_lists_workspace_bytes(int64_t n, int32_t n_batch, int64_t patch_size) {
  if (n < 0 || n_batch < 0 || patch_size < 1) return -1;
  return serial_ws(nullptr, n, n_batch, patch_size).bytes;
}

int me_attn_patch_lists(const int32_t *coords, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                        const int32_t *bbox_min, int32_t depth, int32_t batch_max, int32_t order, int32_t n_batch,
                        int64_t patch_size, int32_t *seg_ptr, int32_t *seg_rows, int32_t *blk_tab, int32_t *row_patch,
                        void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(ncol >= 2 && ncol <= ME_MAX_DIM + 1, "invalid coordinate size");
  ME_CHECK(n >= 0 && n < (1ll << 31) && n_batch >= 0, "number of rows must fit in int32");
  ME_CHECK(patch_size >= 1, "patch_size must be at least 1");
  ME_CHECK(order >= 0 && order <= 3, "order must be 0 (z), 1 (z_trans), 2 (hilbert) or 3 (hilbert_trans)");
  ME_CHECK(depth >= 0 && depth <= 31 && batch_max >= 0, "bad depth or batch index");
  const int D = ncol - 1;
  const int batch_bits = bits_of((uint64_t)(batch_max > n_batch ? batch_max : n_batch));
  ME_CHECK(D * depth + batch_bits <= 63, "the serialisation key (D * depth code bits + the batch bits) must fit in 63 bits");
  ME_CHECK(n == 0 || n_batch >= 1, "rows without an instance");
  const int64_t n_seg = serial_n_seg(n, n_batch, patch_size), n_entries = ceil_div(n, kAttnBlock) + n_seg;
  ME_CHECK(n_seg < (1ll << 31), "too many segments");
  ME_CHECK(workspace_bytes >= me_attn_patch_lists_workspace_bytes(n, n_batch, patch_size), "workspace too small");
  ME_CHECK(seg_ptr != nullptr && blk_tab != nullptr, "seg_ptr and blk_tab must be given");
  ME_HIP(hipMemsetAsync(blk_tab, 0xff, (size_t)n_entries * 8, stream));   // segment -1 everywhere
  if (n == 0) {
    ME_HIP(hipMemsetAsync(seg_ptr, 0, (size_t)(n_seg + 1) * 4, stream));
    return 0;
  }
  ME_CHECK(coords != nullptr && seg_rows != nullptr && row_patch != nullptr && workspace != nullptr, "null pointer");
  const SerialWs w = serial_ws(workspace, n, n_batch, patch_size);
  if (int rc = serial_keys(coords, n, ncol, tensor_stride, bbox_min, depth, order, w.keys, stream)) return rc;
  // the significant bytes only: D * depth code bits, then the bits of the largest batch index
  const int key_bits = D * depth + bits_of((uint64_t)batch_max);
  int shifts[8], np = 0;
  for (int s = 0; s < key_bits; s += 8) shifts[np++] = s;
  if (np == 0) shifts[np++] = 0;
  uint64_t *sk = nullptr;
  if (int rc = radix_argsort_u64(w.keys, w.keys_tmp, n, shifts, np, w.order, &sk, w.sort, w.sort_bytes, stream)) return rc;
  const dim3 block(256), grid_n((unsigned)ceil_div(n, 256));
  hipLaunchKernelGGL(k_inst_bounds, grid_n, block, 0, stream, sk, n, D * depth, w.inst_id);
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(w.inst_id, w.inst_id, n, w.total, w.scan, w.scan_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_inst_start, dim3((unsigned)ceil_div((n > n_batch ? n : n_batch) + 1, 256)), block, 0, stream,
                     w.inst_id, n, n_batch, w.inst_start);
  ME_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_inst_patches, dim3((unsigned)ceil_div(n_batch, 256)), block, 0, stream, w.inst_start, n_batch,
                     patch_size, w.inst_m);
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(w.inst_m, w.inst_m, n_batch, w.total, w.scan, w.scan_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_row_patch, grid_n, block, 0, stream, w.order, w.inst_id, w.inst_start, w.inst_m, n, n_batch,
                     patch_size, n_seg, row_patch);
  ME_LAUNCH_CHECK();
  if (int rc = me_csr_from_coo(row_patch, nullptr, nullptr, 0, n, n_seg, seg_ptr, seg_rows, nullptr, w.csr, w.csr_bytes,
                               stream_))
    return rc;
  hipLaunchKernelGGL(k_seg_blocks, dim3((unsigned)ceil_div(n_seg, 256)), block, 0, stream, seg_ptr, n_seg, w.seg_nblk);
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(w.seg_nblk, w.seg_nblk, n_seg, w.total, w.scan, w.scan_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_blk_tab, dim3((unsigned)ceil_div(n_seg, 256)), block, 0, stream, seg_ptr, w.seg_nblk, n_seg,
                     n_entries, blk_tab);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

// ---- window partitions (MinkowskiWindowSelfAttention, ABI 1.21) -----------------------------------------------------------------
// Space is cut into axis-aligned boxes of w_a cells of the tensor stride, the grid anchored at the origin of the coordinate
// system and moved by s_a cells; a row attends inside its box.  With s_a reduced to [0, w_a):
//   cell_a = floor((floor(c_a / t_a) + s_a) / w_a) = floor((c_a + s_a t_a) / (w_a t_a))      (floors towards -inf)
//   k_window_keys     x_a = cell_a - cell_lo_a = (c_a - base_a) / (w_a t_a) with base_a = cell_lo_a w_a t_a - s_a t_a, the
//                     coordinate at which the lowest cell of the bounding box starts: base_a <= c_a, so the division is one
//                     of non-negative numbers; both in 64 bits (c_a - base_a can reach 2^32 + 2^31).
//                     key = (((batch << bits_0 | x_0) << bits_1 | x_1) ...), bits_a the bit count of the largest x_a: integer
//                     order is the lexicographic order of (batch, cell_0 .. cell_{D-1})
//   sort              the library's stable radix sort over the significant key bytes
//   k_inst_bounds (shift 0) + scan
//                     the rank of a sorted position among the distinct keys: its window
//   k_window_scatter  row_window[order[i]] = rank, and the window count W = last rank + 1 to device memory
// me_attn_segment_lists is the tail of me_attn_patch_lists for any segment id per row: me_csr_from_coo, k_seg_blocks, the
// scan and k_blk_tab on the caller's n_seg.
namespace me {

struct WindowGeom {
  int64_t base[ME_MAX_DIM];       // coordinate at which the lowest cell of the bounding box starts
  uint32_t wt[ME_MAX_DIM];        // window size in coordinate units: w_a t_a < 2^31
  uint32_t x_max[ME_MAX_DIM];     // the largest x_a of the bounding box
  int32_t bits[ME_MAX_DIM];       // its bit count
};

template <int NCOL>
__global__ __launch_bounds__(256) void k_window_keys(const int32_t *__restrict__ coords, int64_t n, WindowGeom g,
                                                    uint64_t *__restrict__ keys) {
  constexpr int D = NCOL - 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t *c = coords + i * NCOL;
  uint64_t key = (uint64_t)(uint32_t)c[0];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    // exact for every int32 coordinate and every extent: 64-bit difference, unsigned 64-bit quotient
    const uint64_t x = (uint64_t)((int64_t)c[1 + a] - g.base[a]) / (uint64_t)g.wt[a];
    // (a row outside the bounding box is a caller's error: its cell is clamped so that the key keeps its fields)
    key = (key << g.bits[a]) | (x < (uint64_t)g.x_max[a] ? x : (uint64_t)g.x_max[a]);
  }
  keys[i] = key;
}

__global__ __launch_bounds__(256) void k_window_scatter(const uint32_t *__restrict__ order, const uint32_t *__restrict__ rank,
                                                       int64_t n, int32_t *__restrict__ row_window,
                                                       int32_t *__restrict__ n_windows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = rank[i], row = order[i];
  if (row < (uint32_t)n) row_window[row] = (int32_t)r;
  if (i == n - 1) *n_windows = (int32_t)r + 1;
}

static int64_t floor_div64(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0)) ? 1 : 0); }

struct WindowWs {
  uint64_t *keys, *keys_tmp;
  uint32_t *order, *rank, *total;
  void *scan, *sort;
  int64_t scan_bytes, sort_bytes, bytes;
};
static WindowWs window_ws(void *base, int64_t n) {
  const int64_t m = n < 1 ? 1 : n;
  char *p = reinterpret_cast<char *>(base);
  int64_t o = 0;
  auto take = [&](int64_t bytes) { char *q = p + o; o += align_up(bytes, 256); return q; };
  WindowWs w;
  w.keys = reinterpret_cast<uint64_t *>(take(m * 8));
  w.keys_tmp = reinterpret_cast<uint64_t *>(take(m * 8));
  w.order = reinterpret_cast<uint32_t *>(take(m * 4));
  w.rank = reinterpret_cast<uint32_t *>(take(m * 4));
  w.total = reinterpret_cast<uint32_t *>(take(256));
  w.scan_bytes = scan_workspace_bytes(m);
  w.scan = take(w.scan_bytes);
  w.sort_bytes = radix_argsort_u64_workspace_bytes(m);
  w.sort = take(w.sort_bytes);
  w.bytes = o;
  return w;
}

struct SegmentWs {
  uint32_t *seg_nblk, *total;
  void *scan, *csr;
  int64_t scan_bytes, csr_bytes, bytes;
};
static SegmentWs segment_ws(void *base, int64_t n, int64_t n_seg) {
  const int64_t m = n < 1 ? 1 : n, s = n_seg < 1 ? 1 : n_seg;
  char *p = reinterpret_cast<char *>(base);
  int64_t o = 0;
  auto take = [&](int64_t bytes) { char *q = p + o; o += align_up(bytes, 256); return q; };
  SegmentWs w;
  w.seg_nblk = reinterpret_cast<uint32_t *>(take(s * 4));
  w.total = reinterpret_cast<uint32_t *>(take(256));
  w.scan_bytes = scan_workspace_bytes(s);
  w.scan = take(w.scan_bytes);
  w.csr_bytes = me_csr_from_coo_workspace_bytes(m);
  w.csr = take(w.csr_bytes);
  w.bytes = o;
  return w;
}

}  // namespace me

extern "C" {

int64_t me_attn_window_ids_workspace_bytes(int64_t n) {
  if (n < 0) return -1;
  return window_ws(nullptr, n).bytes;
}

int me_attn_window_ids(const int32_t *coords, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                       const int32_t *window_size, const int32_t *shift, int32_t n_axes, const int32_t *bbox_min,
                       const int32_t *bbox_max, int32_t batch_min, int32_t batch_max, int32_t *row_window,
                       int32_t *n_windows, void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(ncol >= 2 && ncol <= ME_MAX_DIM + 1, "invalid coordinate size");
  ME_CHECK(n_axes == ncol - 1, "window_size and shift take one value per spatial axis");
  ME_CHECK(n >= 0 && n < (1ll << 31), "number of rows must fit in int32");
  ME_CHECK(tensor_stride != nullptr && window_size != nullptr && shift != nullptr, "tensor_stride, window_size and shift must be given");
  ME_CHECK(n == 0 || (bbox_min != nullptr && bbox_max != nullptr), "bbox_min and bbox_max must be given");
  ME_CHECK(n == 0 || (batch_min >= 0 && batch_max >= batch_min), "batch indices must not be negative");
  const int D = ncol - 1;
  WindowGeom g{};
  int key_bits = n > 0 ? bits_of((uint64_t)batch_max) : 0;
  for (int a = 0; a < D; ++a) {
    ME_CHECK(tensor_stride[a] > 0, "the tensor stride must be positive");
    ME_CHECK(window_size[a] >= 1, "window_size must be at least 1");
    const int64_t t = tensor_stride[a], w = window_size[a], wt = w * t;
    ME_CHECK(wt < (1ll << 31), "window_size * tensor_stride must fit in int32");
    const int64_t s = (((int64_t)shift[a] % w) + w) % w, off = s * t;   // the shift modulo the window
    int64_t lo = 0, hi = 0;
    if (n > 0) {
      ME_CHECK(bbox_max[a] >= bbox_min[a], "bbox_max must not be below bbox_min");
      lo = floor_div64((int64_t)bbox_min[a] + off, wt);
      hi = floor_div64((int64_t)bbox_max[a] + off, wt);
    }
    g.base[a] = lo * wt - off;
    g.wt[a] = (uint32_t)wt;
    g.x_max[a] = (uint32_t)(hi - lo);     // <= (2^32 - 1 + wt - 1) / wt < 2^32
    g.bits[a] = bits_of((uint64_t)(hi - lo));
    key_bits += g.bits[a];
  }
  ME_CHECK(key_bits <= 63, "the window key (the cell bits of every axis + the batch bits) must fit in 63 bits");
  ME_CHECK(workspace_bytes >= me_attn_window_ids_workspace_bytes(n), "workspace too small");
  ME_CHECK(n_windows != nullptr, "n_windows must be given");
  if (n == 0) {
    ME_HIP(hipMemsetAsync(n_windows, 0, 4, stream));
    return 0;
  }
  ME_CHECK(coords != nullptr && row_window != nullptr && workspace != nullptr, "null pointer");
  const WindowWs w = window_ws(workspace, n);
  const dim3 block(256), grid_n((unsigned)ceil_div(n, 256));
  ME_DISPATCH_NCOL(ncol, hipLaunchKernelGGL(k_window_keys<NCOL>, grid_n, block, 0, stream, coords, n, g, w.keys));
  ME_LAUNCH_CHECK();
  int shifts[8], np = 0;
  for (int s = 0; s < key_bits; s += 8) shifts[np++] = s;
  if (np == 0) shifts[np++] = 0;
  uint64_t *sk = nullptr;
  if (int rc = radix_argsort_u64(w.keys, w.keys_tmp, n, shifts, np, w.order, &sk, w.sort, w.sort_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_inst_bounds, grid_n, block, 0, stream, sk, n, 0, w.rank);   // 1 where the next key differs
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(w.rank, w.rank, n, w.total, w.scan, w.scan_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_window_scatter, grid_n, block, 0, stream, w.order, w.rank, n, row_window, n_windows);
  ME_LAUNCH_CHECK();
  return 0;
}

int64_t me_attn_segment_lists_workspace_bytes(int64_t n, int64_t n_seg) {
  if (n < 0 || n_seg < 0) return -1;
  return segment_ws(nullptr, n, n_seg).bytes;
}

int me_attn_segment_lists(const int32_t *row_segment, int64_t n, int64_t n_seg, int32_t *seg_ptr, int32_t *seg_rows,
                          int32_t *blk_tab, void *workspace, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(n >= 0 && n < (1ll << 31), "number of rows must fit in int32");
  ME_CHECK(n_seg >= 0 && n_seg < (1ll << 31), "too many segments");
  ME_CHECK(n == 0 || n_seg >= 1, "rows without a segment");
  ME_CHECK(workspace_bytes >= me_attn_segment_lists_workspace_bytes(n, n_seg), "workspace too small");
  ME_CHECK(seg_ptr != nullptr && (blk_tab != nullptr || n_seg == 0), "seg_ptr and blk_tab must be given");
  const int64_t n_entries = ceil_div(n, kAttnBlock) + n_seg;
  if (n_entries > 0) ME_HIP(hipMemsetAsync(blk_tab, 0xff, (size_t)n_entries * 8, stream));   // segment -1 everywhere
  if (n == 0) {
    ME_HIP(hipMemsetAsync(seg_ptr, 0, (size_t)(n_seg + 1) * 4, stream));
    return 0;
  }
  ME_CHECK(row_segment != nullptr && seg_rows != nullptr && workspace != nullptr, "null pointer");
  const SegmentWs w = segment_ws(workspace, n, n_seg);
  if (int rc = me_csr_from_coo(row_segment, nullptr, nullptr, 0, n, n_seg, seg_ptr, seg_rows, nullptr, w.csr, w.csr_bytes,
                               stream_))
    return rc;
  const dim3 block(256), grid_s((unsigned)ceil_div(n_seg, 256));
  hipLaunchKernelGGL(k_seg_blocks, grid_s, block, 0, stream, seg_ptr, n_seg, w.seg_nblk);
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(w.seg_nblk, w.seg_nblk, n_seg, w.total, w.scan, w.scan_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_blk_tab, grid_s, block, 0, stream, seg_ptr, w.seg_nblk, n_seg, n_entries, blk_tab);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
