// Dense <-> sparse conversion (SparseTensor.dense / ME.to_sparse / ME.to_sparse_all / ME.dense_coordinates; reference:
// MinkowskiEngine/MinkowskiSparseTensor.py:460-557 and MinkowskiOps.py:246-348, both torch indexing there).
//
// One family of moves: C-wide feature rows between a row-major matrix [N, C] and a strided box [outer, C, inner].  A cell is
// (o, i), its linear index o * inner + i — which is also its linear index over (B, X1, .., XD), wherever the channel axis
// sits in the layout, so cell indices, the grid and the coordinates never depend on the layout; only the movers take
// `inner`.  Values are moved as raw 2 / 4 / 8-byte words (bf16 / fp32 / float64): copies, no arithmetic, no atomics.
//
//   k_cell_index      coords -> cell[N] (-1 and a raised flag for a row outside the box, on either side)
//   k_grid_scatter    cell[N] -> grid[cells] (row of every cell, -1 = empty; unique coordinates: race-free)
//   k_tile_to_box     cell-stationary rows -> box: 64 consecutive cells x 64 channels per pass through LDS; rows are read as
//                     contiguous C-vectors, the box is written coalesced along `inner`, zeros included: one pass, no memset
//   k_tile_to_rows    the same tile backwards: box read coalesced, rows written as contiguous C-vectors
//   k_row_move        row-stationary movers, both directions (one wave per row; box accesses `inner` apart): the low-occupancy
//                     side of me_dense_policy
//   k_occupied_mask / k_occupied_fill   kept cells of a box in ascending cell order: wave ballots, a scan of the wave counts
//   k_all_coords      coordinates of every cell in cell order
#include "common.hpp"

namespace me {
namespace dense {

constexpr int kThreads = 256;
constexpr int kT = 64;          // cells per tile
constexpr int kCC = 64;         // channels per pass
constexpr int kPad = kT + 1;    // LDS row pitch in elements: column and row walks are both conflict-free

struct Box {
  int32_t d;                        // spatial dimensions
  int64_t dim[ME_MAX_DIM + 1];      // B, X1 .. XD
  int32_t mn[ME_MAX_DIM];           // min_coordinate
  int32_t dv[ME_MAX_DIM];           // divisor: the tensor stride when the box is contracted, else 1
};

__global__ __launch_bounds__(kThreads) void k_cell_index(const int32_t *__restrict__ coords, int64_t n, Box s,
                                                          int64_t *__restrict__ cell, int32_t *__restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const int32_t *c = coords + r * (s.d + 1);
  int64_t lin = c[0];
  bool ok = lin >= 0 && lin < s.dim[0];
#pragma unroll
  for (int k = 0; k < ME_MAX_DIM; ++k) {
    if (k < s.d) {
      const int64_t v = (int64_t)c[1 + k] - s.mn[k];
      int64_t q = v / s.dv[k];
      if (v % s.dv[k] != 0 && v < 0) --q;       // floor, as torch's `//`
      ok = ok && q >= 0 && q < s.dim[1 + k];
      lin = lin * s.dim[1 + k] + q;
    }
  }
  cell[r] = ok ? lin : -1;
  if (!ok) *flag = 1;
}

__global__ __launch_bounds__(kThreads) void k_grid_scatter(const int64_t *__restrict__ cell, int64_t n, int64_t n_cells,
                                                            int32_t *__restrict__ grid) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const int64_t c = cell[r];
  if (c >= 0 && c < n_cells) grid[c] = (int32_t)r;
}

template <typename T>
struct alignas(sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16) Vec4 {
  T v[4];
};

// Row and box offset of the 64 cells of a tile; -> whether any of them has a row.
template <bool IDENTITY>
__device__ __forceinline__ int tile_setup(const int32_t *__restrict__ grid, int64_t n_rows, int64_t n_cells, int32_t C,
                                          int64_t inner, int64_t cell0, int32_t *s_row, int64_t *s_base) {
  const int tid = threadIdx.x;
  int32_t r = -1;
  if (tid < kT) {
    const int64_t cell = cell0 + tid;
    int64_t base = -1;
    if (cell < n_cells) {
      r = IDENTITY ? (int32_t)cell : grid[cell];
      if (r >= n_rows) r = -1;
      const int64_t o = cell / inner;
      base = o * C * inner + (cell - o * inner);
    }
    s_row[tid] = r;
    s_base[tid] = base;
  }
  return __syncthreads_or(r >= 0);
}

// MODE 0: 4 cells per lane, 4-element vector accesses (inner % 4 == 0, box 16-byte aligned); 1: cell fastest, scalar;
// 2: channel fastest (small `inner`, channels-last boxes)
template <typename T, int MODE, bool TO_BOX>
__device__ __forceinline__ void tile_box_pass(T *__restrict__ box, T *tile, const int64_t *s_base, int cc, int c0,
                                              int64_t inner) {
  const int tid = threadIdx.x;
  if constexpr (MODE == 0) {
    const int j4 = (tid & 15) * 4;
    const int64_t base = s_base[j4];
    if (base < 0) return;
    for (int c = tid >> 4; c < cc; c += kThreads / 16) {
      Vec4<T> *p = reinterpret_cast<Vec4<T> *>(box + base + (int64_t)(c0 + c) * inner);
      T *t = tile + c * kPad + j4;
      if constexpr (TO_BOX) {
        Vec4<T> v;
        v.v[0] = t[0]; v.v[1] = t[1]; v.v[2] = t[2]; v.v[3] = t[3];
        *p = v;
      } else {
        const Vec4<T> v = *p;
        t[0] = v.v[0]; t[1] = v.v[1]; t[2] = v.v[2]; t[3] = v.v[3];
      }
    }
  } else if constexpr (MODE == 1) {
    const int j = tid & (kT - 1);
    const int64_t base = s_base[j];
    if (base < 0) return;
    for (int c = tid >> 6; c < cc; c += kThreads / kT) {
      T *p = box + base + (int64_t)(c0 + c) * inner;
      if constexpr (TO_BOX) *p = tile[c * kPad + j];
      else tile[c * kPad + j] = *p;
    }
  } else {
    const int c = tid & (kCC - 1);
    if (c >= cc) return;
    for (int j = tid >> 6; j < kT; j += kThreads / kCC) {
      const int64_t base = s_base[j];
      if (base < 0) continue;
      T *p = box + base + (int64_t)(c0 + c) * inner;
      if constexpr (TO_BOX) *p = tile[c * kPad + j];
      else tile[c * kPad + j] = *p;
    }
  }
}

// rows of the tile's cells <-> LDS, channel fastest: every row segment is one contiguous run of cc elements
template <typename T, bool TO_ROWS>
__device__ __forceinline__ void tile_rows_pass(T *__restrict__ rows, T *tile, const int32_t *s_row, int cc, int c0,
                                               int32_t C) {
  const int tid = threadIdx.x;
  const int c = tid & (kCC - 1);
  if (c >= cc) return;
  for (int j = tid >> 6; j < kT; j += kThreads / kCC) {
    const int32_t r = s_row[j];
    if constexpr (TO_ROWS) {
      if (r >= 0) rows[(int64_t)r * C + c0 + c] = tile[c * kPad + j];
    } else {
      tile[c * kPad + j] = r >= 0 ? rows[(int64_t)r * C + c0 + c] : T(0);
    }
  }
}

template <typename T, int MODE, bool IDENTITY>
__global__ __launch_bounds__(kThreads) void k_tile_to_box(const T *__restrict__ rows, const int32_t *__restrict__ grid,
                                                           int64_t n_rows, int64_t n_cells, int32_t C, int64_t inner,
                                                           T *__restrict__ box) {
  __shared__ T tile[kCC * kPad];
  __shared__ int64_t s_base[kT];
  __shared__ int32_t s_row[kT];
  const int64_t cell0 = (int64_t)blockIdx.x * kT;
  const int any = tile_setup<IDENTITY>(grid, n_rows, n_cells, C, inner, cell0, s_row, s_base);
  if (!any) {                       // an empty tile: zeros once, stored for every pass
    for (int i = threadIdx.x; i < kCC * kPad; i += kThreads) tile[i] = T(0);
    __syncthreads();
  }
  for (int c0 = 0; c0 < C; c0 += kCC) {
    const int cc = C - c0 < kCC ? C - c0 : kCC;
    if (any) {
      tile_rows_pass<T, false>(const_cast<T *>(rows), tile, s_row, cc, c0, C);
      __syncthreads();
    }
    tile_box_pass<T, MODE, true>(box, tile, s_base, cc, c0, inner);
    if (any) __syncthreads();
  }
}

template <typename T, int MODE, bool IDENTITY>
__global__ __launch_bounds__(kThreads) void k_tile_to_rows(const T *__restrict__ box, const int32_t *__restrict__ grid,
                                                            int64_t n_rows, int64_t n_cells, int32_t C, int64_t inner,
                                                            T *__restrict__ rows) {
  __shared__ T tile[kCC * kPad];
  __shared__ int64_t s_base[kT];
  __shared__ int32_t s_row[kT];
  const int64_t cell0 = (int64_t)blockIdx.x * kT;
  const int any = tile_setup<IDENTITY>(grid, n_rows, n_cells, C, inner, cell0, s_row, s_base);
  if (!any) return;                 // no row reads from this tile
  for (int c0 = 0; c0 < C; c0 += kCC) {
    const int cc = C - c0 < kCC ? C - c0 : kCC;
    tile_box_pass<T, MODE, false>(const_cast<T *>(box), tile, s_base, cc, c0, inner);
    __syncthreads();
    tile_rows_pass<T, true>(rows, tile, s_row, cc, c0, C);
    __syncthreads();
  }
}

// row-stationary: one wave per row, lanes over the channels
template <typename T, bool TO_BOX>
__global__ __launch_bounds__(kThreads) void k_row_move(T *__restrict__ rows, const int64_t *__restrict__ cell, int64_t n,
                                                        int64_t n_cells, int32_t C, int64_t inner, T *__restrict__ box) {
  const int64_t r = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t cl = cell ? cell[r] : r;
  const bool ok = cl >= 0 && cl < n_cells;
  if (!ok && TO_BOX) return;        // a row outside the box is never written
  const int64_t o = ok ? cl / inner : 0;
  T *b = box + o * C * inner + (cl - o * inner);
  for (int c = lane_id(); c < C; c += kWave) {
    if constexpr (TO_BOX) b[(int64_t)c * inner] = rows[r * C + c];
    else rows[r * C + c] = ok ? b[(int64_t)c * inner] : T(0);
  }
}

// a cell is kept when any of its channels is not +-0 (== `abs(x).sum(channel) != 0`: a sum of non-negative numbers is zero
// only when every term is; NaN != 0 keeps the cell as in torch): all bits but the sign bit, so one kernel per word size
template <typename T>
__global__ __launch_bounds__(kThreads) void k_occupied_mask(const T *__restrict__ box, int64_t n_cells, int32_t C,
                                                             int64_t inner, uint64_t *__restrict__ wmask,
                                                             uint32_t *__restrict__ wcount) {
  const int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  bool keep = false;
  if (cell < n_cells) {
    const int64_t o = cell / inner;
    const T *p = box + o * C * inner + (cell - o * inner);
    T acc = 0;
    for (int c = 0; c < C; ++c) acc |= p[(int64_t)c * inner];
    keep = (T)(acc << 1) != 0;
  }
  const unsigned long long m = __ballot(keep);
  if (lane_id() == 0 && (cell >> 6) < ((n_cells + 63) >> 6)) {
    wmask[cell >> 6] = m;
    wcount[cell >> 6] = (uint32_t)__popcll(m);
  }
}

__device__ __forceinline__ void decompose(uint32_t cell, const Box &s, int32_t *__restrict__ out) {
  uint32_t rem = cell;
#pragma unroll
  for (int k = ME_MAX_DIM; k >= 1; --k) {
    if (k <= s.d) {
      const uint32_t dk = (uint32_t)s.dim[k];
      const uint32_t q = rem / dk;
      out[k] = (int32_t)(rem - q * dk);
      rem = q;
    }
  }
  out[0] = (int32_t)rem;
}

__global__ __launch_bounds__(kThreads) void k_occupied_fill(const uint64_t *__restrict__ wmask,
                                                             const uint32_t *__restrict__ woffs, int64_t n_cells, Box s,
                                                             int32_t *__restrict__ coords, int64_t *__restrict__ cell_out) {
  const int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (cell >= n_cells) return;
  const unsigned long long m = wmask[cell >> 6];
  const int lane = (int)(cell & 63);
  if (!((m >> lane) & 1ull)) return;
  const int64_t pos = (int64_t)woffs[cell >> 6] + __popcll(m & ((1ull << lane) - 1ull));
  cell_out[pos] = cell;
  decompose((uint32_t)cell, s, coords + pos * (s.d + 1));
}

__global__ __launch_bounds__(kThreads) void k_all_coords(int64_t n_cells, Box s, int32_t *__restrict__ coords) {
  const int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (cell >= n_cells) return;
  decompose((uint32_t)cell, s, coords + cell * (s.d + 1));
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static int make_box(int32_t ncol, const int64_t *shape, const int32_t *mn, const int32_t *dv, Box *b, int64_t *n_cells) {
  ME_CHECK(ncol >= 2 && ncol <= ME_MAX_DIM + 1, "coordinate size (D+1) must be in [2, 8]");
  ME_CHECK(shape != nullptr, "shape is required");
  b->d = ncol - 1;
  int64_t cells = 1;
  for (int k = 0; k <= ME_MAX_DIM; ++k) {
    b->dim[k] = k < ncol ? shape[k] : 1;
    ME_CHECK(b->dim[k] >= 0 && b->dim[k] < (1ll << 31), "box extents must be in [0, 2^31)");
    cells *= b->dim[k];
    ME_CHECK(cells < (1ll << 40), "box too large");
  }
  for (int k = 0; k < ME_MAX_DIM; ++k) {
    b->mn[k] = (mn && k < ncol - 1) ? mn[k] : 0;
    b->dv[k] = (dv && k < ncol - 1) ? dv[k] : 1;
    ME_CHECK(b->dv[k] > 0, "divisors must be positive");
  }
  *n_cells = cells;
  return 0;
}

static inline unsigned blocks_for(int64_t n, int per) { return (unsigned)ceil_div(n, per); }

template <typename T, bool TO_BOX>
static int tile_launch(const void *rows, const int32_t *grid, int64_t n, int64_t n_cells, int32_t c, int64_t inner,
                       const void *box, hipStream_t stream) {
  const bool vec = inner % 4 == 0 && (reinterpret_cast<uintptr_t>(box) & 15) == 0;
  const int mode = vec ? 0 : (inner >= 16 ? 1 : 2);
  const dim3 g(blocks_for(n_cells, kT)), b(kThreads);
  T *rw = reinterpret_cast<T *>(const_cast<void *>(rows));
  T *bx = reinterpret_cast<T *>(const_cast<void *>(box));
#define ME_DENSE_TILE(MODE, ID)                                                                                           \
  do {                                                                                                                    \
    if constexpr (TO_BOX) hipLaunchKernelGGL((k_tile_to_box<T, MODE, ID>), g, b, 0, stream, rw, grid, n, n_cells, c, inner, bx); \
    else hipLaunchKernelGGL((k_tile_to_rows<T, MODE, ID>), g, b, 0, stream, bx, grid, n, n_cells, c, inner, rw);           \
  } while (0)
  if (grid == nullptr) {
    if (mode == 0) ME_DENSE_TILE(0, true); else if (mode == 1) ME_DENSE_TILE(1, true); else ME_DENSE_TILE(2, true);
  } else {
    if (mode == 0) ME_DENSE_TILE(0, false); else if (mode == 1) ME_DENSE_TILE(1, false); else ME_DENSE_TILE(2, false);
  }
#undef ME_DENSE_TILE
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int move(bool to_box, const void *rows, const int64_t *cell, const int32_t *grid, int64_t n, int64_t outer,
                int32_t c, int64_t inner, const void *box, int32_t policy, hipStream_t stream) {
  const int64_t n_cells = outer * inner;
  const bool identity = cell == nullptr && grid == nullptr;
  if (policy == 0) policy = (grid != nullptr || identity) ? ME_DENSE_CELL_STATIONARY : ME_DENSE_ROW_STATIONARY;
  if (policy == ME_DENSE_CELL_STATIONARY) {
    ME_CHECK(grid != nullptr || identity, "the cell-stationary movers need the grid (me_dense_grid)");
    if (n_cells == 0 || (!to_box && n == 0)) return 0;
    return to_box ? tile_launch<T, true>(rows, grid, n, n_cells, c, inner, box, stream)
                  : tile_launch<T, false>(rows, grid, n, n_cells, c, inner, box, stream);
  }
  ME_CHECK(cell != nullptr || identity, "the row-stationary movers need the cell index of every row");
  if (to_box && n_cells > 0) ME_HIP(hipMemsetAsync(const_cast<void *>(box), 0, (size_t)n_cells * c * sizeof(T), stream));
  if (n == 0 || n_cells == 0) return 0;
  const dim3 g(blocks_for(n, kThreads / kWave)), b(kThreads);
  T *rw = reinterpret_cast<T *>(const_cast<void *>(rows));
  T *bx = reinterpret_cast<T *>(const_cast<void *>(box));
  if (to_box) hipLaunchKernelGGL((k_row_move<T, true>), g, b, 0, stream, rw, cell, n, n_cells, c, inner, bx);
  else hipLaunchKernelGGL((k_row_move<T, false>), g, b, 0, stream, rw, cell, n, n_cells, c, inner, bx);
  ME_LAUNCH_CHECK();
  return 0;
}

static int move_any(bool to_box, const void *rows, int32_t elem_bytes, const int64_t *cell, const int32_t *grid, int64_t n,
                    int64_t outer, int32_t c, int64_t inner, const void *box, int32_t policy, hipStream_t stream) {
  ME_CHECK(n >= 0 && n < (1ll << 31) && outer >= 0 && inner >= 1 && c >= 1, "invalid sizes");
  ME_CHECK(outer < (1ll << 40) / inner, "box too large");
  ME_CHECK(policy >= 0 && policy <= 2, "policy must be 0 (auto), ME_DENSE_ROW_STATIONARY or ME_DENSE_CELL_STATIONARY");
  if (cell == nullptr && grid == nullptr) ME_CHECK(n == outer * inner, "identity moves need one row per cell");
  switch (elem_bytes) {
    case 2: return move<uint16_t>(to_box, rows, cell, grid, n, outer, c, inner, box, policy, stream);
    case 4: return move<uint32_t>(to_box, rows, cell, grid, n, outer, c, inner, box, policy, stream);
    case 8: return move<uint64_t>(to_box, rows, cell, grid, n, outer, c, inner, box, policy, stream);
    default: ME_FAIL("element size must be 2 (bf16), 4 (fp32) or 8 (float64) bytes");
  }
}

struct OccWs {
  uint64_t *wmask;
  uint32_t *woffs, *total;
  void *scan_ws;
  int64_t n_waves;
};
static int64_t occ_ws_bytes(int64_t n_cells) {
  const int64_t w = ceil_div(n_cells > 0 ? n_cells : 1, 64);
  return align_up(w * 8, 256) + align_up(w * 4, 256) + 256 + scan_workspace_bytes(w);
}
static OccWs occ_ws(void *ws, int64_t n_cells) {
  const int64_t w = ceil_div(n_cells > 0 ? n_cells : 1, 64);
  char *p = reinterpret_cast<char *>(ws);
  OccWs o;
  o.wmask = reinterpret_cast<uint64_t *>(p); p += align_up(w * 8, 256);
  o.woffs = reinterpret_cast<uint32_t *>(p); p += align_up(w * 4, 256);
  o.total = reinterpret_cast<uint32_t *>(p); p += 256;
  o.scan_ws = p;
  o.n_waves = w;
  return o;
}

}  // namespace dense
}  // namespace me

using namespace me;
using namespace me::dense;

extern "C" {

int me_dense_policy(int64_t n, int64_t n_cells, int32_t c, int32_t elem_bytes, int32_t to_box) {
  // Cost in bytes at the streaming rate.  Towards the rows (to_box = 0) it is the bytes moved: a cell-stationary pass reads
  // the whole box, writes the rows and reads and builds the grid (8 bytes per cell); a row-stationary pass touches one
  // 64-byte sector per element.  Towards the box both shapes write the whole box, and the measured rates decide
  // (scripts/dense_bench.py): the zero fill streams at the full rate, the tile kernel stores its 256-byte runs,
  // one per channel plane, at about 0.4 of it on boxes beyond the cache (factor 2.5), and a scattered element costs about
  // 40 ps = 256 bytes.  The crossover is an occupancy of about 0.023 for fp32 and 0.012 for bf16.
  const double e = elem_bytes, rows = (double)n * c * e, box = (double)n_cells * c * e;
  const double cell_cost = (to_box ? 2.5 : 1.0) * box + rows + 8.0 * (double)n_cells;
  const double row_cost = (to_box ? box : 0.0) + rows + (to_box ? 256.0 : 64.0) * (double)n * c;
  return cell_cost <= row_cost ? ME_DENSE_CELL_STATIONARY : ME_DENSE_ROW_STATIONARY;
}

int me_dense_cell_index(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *min_coord,
                        const int32_t *divisor, const int64_t *shape, int64_t *cell_dev, int32_t *flag_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  Box b;
  int64_t n_cells = 0;
  if (int rc = make_box(ncol, shape, min_coord, divisor, &b, &n_cells)) return rc;
  ME_CHECK(flag_dev != nullptr, "flag_dev is required");
  ME_HIP(hipMemsetAsync(flag_dev, 0, 4, stream));
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_cell_index, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, coords_dev, n, b, cell_dev,
                     flag_dev);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_dense_grid(const int64_t *cell_dev, int64_t n, int64_t n_cells, int32_t *grid_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(n >= 0 && n < (1ll << 31) && n_cells >= 0, "invalid sizes");
  if (n_cells == 0) return 0;
  ME_HIP(hipMemsetAsync(grid_dev, 0xff, (size_t)n_cells * 4, stream));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_grid_scatter, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, cell_dev, n, n_cells,
                     grid_dev);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_dense_rows_to_box(const void *rows_dev, int32_t elem_bytes, const int64_t *cell_dev, const int32_t *grid_dev,
                         int64_t n, int64_t outer, int32_t c, int64_t inner, void *box_dev, int32_t policy, void *stream) {
  return move_any(true, rows_dev, elem_bytes, cell_dev, grid_dev, n, outer, c, inner, box_dev, policy, (hipStream_t)stream);
}

int me_dense_box_to_rows(const void *box_dev, int32_t elem_bytes, const int64_t *cell_dev, const int32_t *grid_dev,
                         int64_t n, int64_t outer, int32_t c, int64_t inner, void *rows_dev, int32_t policy, void *stream) {
  return move_any(false, rows_dev, elem_bytes, cell_dev, grid_dev, n, outer, c, inner, box_dev, policy, (hipStream_t)stream);
}

int64_t me_dense_occupied_workspace_bytes(int64_t n_cells) { return occ_ws_bytes(n_cells); }

int me_dense_occupied_count(const void *box_dev, int32_t elem_bytes, int64_t outer, int32_t c, int64_t inner,
                            void *workspace_dev, int64_t workspace_bytes, int64_t *n_occupied, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(outer >= 0 && inner >= 1 && c >= 1 && n_occupied != nullptr, "invalid arguments");
  ME_CHECK(outer < (1ll << 31) / inner, "the box must have fewer than 2^31 cells");
  const int64_t n_cells = outer * inner;
  *n_occupied = 0;
  if (n_cells == 0) return 0;
  ME_CHECK(workspace_bytes >= occ_ws_bytes(n_cells), "workspace too small");
  const OccWs w = occ_ws(workspace_dev, n_cells);
  const dim3 g(blocks_for(n_cells, kThreads)), b(kThreads);
  switch (elem_bytes) {
    case 2: hipLaunchKernelGGL(k_occupied_mask<uint16_t>, g, b, 0, stream, (const uint16_t *)box_dev, n_cells, c, inner, w.wmask, w.woffs); break;
    case 4: hipLaunchKernelGGL(k_occupied_mask<uint32_t>, g, b, 0, stream, (const uint32_t *)box_dev, n_cells, c, inner, w.wmask, w.woffs); break;
    case 8: hipLaunchKernelGGL(k_occupied_mask<uint64_t>, g, b, 0, stream, (const uint64_t *)box_dev, n_cells, c, inner, w.wmask, w.woffs); break;
    default: ME_FAIL("element size must be 2 (bf16), 4 (fp32) or 8 (float64) bytes");
  }
  ME_LAUNCH_CHECK();
  if (int rc = exclusive_scan_u32(w.woffs, w.woffs, w.n_waves, w.total, w.scan_ws, scan_workspace_bytes(w.n_waves), stream))
    return rc;
  uint32_t h = 0;
  ME_HIP(hipMemcpyAsync(&h, w.total, 4, hipMemcpyDeviceToHost, stream));
  ME_HIP(hipStreamSynchronize(stream));
  *n_occupied = h;
  return 0;
}

int me_dense_occupied_fill(const void *workspace_dev, int64_t workspace_bytes, int32_t ncol, const int64_t *shape,
                           int32_t *coords_dev, int64_t *cell_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  Box b;
  int64_t n_cells = 0;
  if (int rc = make_box(ncol, shape, nullptr, nullptr, &b, &n_cells)) return rc;
  ME_CHECK(n_cells < (1ll << 31), "the box must have fewer than 2^31 cells");
  if (n_cells == 0) return 0;
  ME_CHECK(workspace_bytes >= occ_ws_bytes(n_cells), "workspace too small");
  const OccWs w = occ_ws(const_cast<void *>(workspace_dev), n_cells);
  hipLaunchKernelGGL(k_occupied_fill, dim3(blocks_for(n_cells, kThreads)), dim3(kThreads), 0, stream, w.wmask, w.woffs,
                     n_cells, b, coords_dev, cell_dev);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_dense_all_coords(int32_t ncol, const int64_t *shape, int32_t *coords_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  Box b;
  int64_t n_cells = 0;
  if (int rc = make_box(ncol, shape, nullptr, nullptr, &b, &n_cells)) return rc;
  ME_CHECK(n_cells < (1ll << 31), "the box must have fewer than 2^31 cells");
  if (n_cells == 0) return 0;
  hipLaunchKernelGGL(k_all_coords, dim3(blocks_for(n_cells, kThreads)), dim3(kThreads), 0, stream, n_cells, b, coords_dev);
  ME_LAUNCH_CHECK();
  return 0;
}

__attribute__((visibility("hidden"))) void me_preload_dense(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::dense::k_cell_index));
}

}  // extern "C"
