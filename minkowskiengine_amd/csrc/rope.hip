// Rotary position embedding from voxel coordinates for gfx950 (MI355X): q and k of an attention layer are rotated pair by
// pair by angles taken from the coordinates of their row, after which <q_i, k_j> depends on c_i - c_j only (the 3-D RoPE
// of sparse generative transformers; definition in include/me_amd.h, ABI 1.22).
//
//   * k_rope_table: one thread per (row, pair).  theta = ((double)c_a / (double)u_a) * omega_j, the range reduction and
//     sin / cos are in double and the two values are rounded once into the table [n][P][2] = (cos, sin) (fp32, or float64
//     for float64 features).  omega_j = base^(-j / m) comes from the host (pow in double, once per call) in the kernel
//     arguments.  Runs once per (map, d, base, unit, table dtype): the host layers cache the table.
//   * k_rope_apply: one thread per (row, 16-byte piece of the row), or per (row, pair) where the operands do not allow
//     16-byte pieces.  A piece of x (8 bf16, 4 fp32, 2 double) takes the matching contiguous run of the table; heads repeat
//     the same P entries.  Two multiplies and two fused multiply-adds per pair, written out explicitly so that both paths
//     and every instantiation round in the same places; bf16 rows are widened to fp32, rotated there and rounded once:
//     rope(x_bf16) = bf16(rope(float(x_bf16))) bit for bit.  No transcendental, no LDS, no atomics, nothing read back.
//     Grid capped at 2048 workgroups with a grid-stride loop.
// Byte model of an apply call: n * heads * d * sizeof(T) read + written, n * d * sizeof(table value) of table.
#include "piece.hpp"

#include <cmath>

namespace me {
namespace rope {

constexpr int kMaxPairs = ME_ROPE_MAX_PAIRS;
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 workgroups: the rest is a grid-stride loop

// host values of one table: omega_j for j < m, and the unit of every axis as a double
struct TableArgs {
  double omega[kMaxPairs];
  double unit[ME_MAX_DIM];
};

template <typename TT>
__global__ __launch_bounds__(256) void k_rope_table(const int32_t *__restrict__ coords, int64_t n, int ncol, int P, int m,
                                                   const TableArgs args, TT *__restrict__ table) {
  const int64_t total = n * P, step = (int64_t)gridDim.x * blockDim.x;
  const int rotated = (ncol - 1) * m;   // pairs beyond pass through
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
    const int64_t row = idx / P;
    const int p = (int)(idx - row * P);
    double cs = 1.0, sn = 0.0;
    if (p < rotated) {
      const int a = p / m, j = p - a * m;
      const double t = (double)coords[row * ncol + 1 + a] / args.unit[a];
      const double theta = t * args.omega[j];
      sincos(theta, &sn, &cs);
    }
    typedef TT tt2 __attribute__((ext_vector_type(2)));
    tt2 o;
    o.x = (TT)cs;
    o.y = (TT)sn;
    *reinterpret_cast<tt2 *>(table + 2 * idx) = o;
  }
}

// (x0, x1) -> (x0 c - x1 s, x0 s + x1 c): one product and one fused multiply-add per output, the same in every path
template <typename A>
__device__ __forceinline__ void rotate(A x0, A x1, A c, A s, A &y0, A &y1) {
  if constexpr (sizeof(A) == 8) {
    y0 = __builtin_fma(x0, c, -(x1 * s));
    y1 = __builtin_fma(x0, s, x1 * c);
  } else {
    y0 = __builtin_fmaf(x0, c, -(x1 * s));
    y1 = __builtin_fmaf(x0, s, x1 * c);
  }
}

// V == 16 / sizeof(T): the vector path, a thread owns V consecutive channels (V / 2 pairs) of one row and the V table
// values that go with them.  V == 2 with PAIR: the pair path, element accesses to x and y, one 2-value access to the table.
// A: the type of the arithmetic and of the table.  `small`: n * pieces < 2^32, the row comes from a 32-bit division.
template <typename T, typename A, int V, bool PAIR>
__global__ __launch_bounds__(256) void k_rope_apply(const T *__restrict__ x, int64_t x_stride, T *__restrict__ y,
                                                   int64_t y_stride, int64_t n, int c, int d,
                                                   const A *__restrict__ table, A sign, bool small) {
  const int pieces = c / V;
  const int64_t total = n * pieces, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
    const int64_t row = small ? (int64_t)((uint32_t)idx / (uint32_t)pieces) : idx / pieces;
    const int ch = (int)(idx - row * pieces) * V;
    const int hc = ch % d;   // channel inside the head: the table run starts at the same offset (2 values per pair)
    const A *trow = table + row * d + hc;
    Piece<V, A> xv, tv, o;
    if constexpr (PAIR) {
      xv.v[0] = (A)x[row * x_stride + ch];
      xv.v[1] = (A)x[row * x_stride + ch + 1];
      tv = load_piece<A, 2, A>(trow);
    } else {
      xv = load_piece<T, V, A>(x + row * x_stride + ch);
      constexpr int TV = 16 / (int)sizeof(A);   // table values per 16-byte load
#pragma unroll
      for (int q = 0; q < V / TV; ++q) {
        const Piece<TV, A> t = load_piece<A, TV, A>(trow + q * TV);
#pragma unroll
        for (int j = 0; j < TV; ++j) tv.v[q * TV + j] = t.v[j];
      }
    }
#pragma unroll
    for (int j = 0; j < V; j += 2) rotate<A>(xv.v[j], xv.v[j + 1], tv.v[j], sign * tv.v[j + 1], o.v[j], o.v[j + 1]);
    if constexpr (PAIR) {
      y[row * y_stride + ch] = (T)o.v[0];
      y[row * y_stride + ch + 1] = (T)o.v[1];
    } else {
      store_piece<T, V, A>(y + row * y_stride + ch, o);
    }
  }
}

inline unsigned capped_grid(int64_t items) {
  const int64_t blocks = ceil_div(items, 256);
  return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

template <typename T, typename A>
int apply(const T *x, int64_t x_stride, T *y, int64_t y_stride, int64_t n, int c, int d, const A *table, int sign,
          hipStream_t stream) {
  constexpr int W = 16 / (int)sizeof(T);
  const bool vec = d % W == 0 && x_stride % W == 0 && y_stride % W == 0 && aligned({x, y, table}, 16);
  const int v = vec ? W : 2;
  const int64_t total = n * (c / v);
  const bool small = total < (1ll << 32);
  const dim3 grid(capped_grid(total)), block(256);
  if (vec)
    hipLaunchKernelGGL((k_rope_apply<T, A, W, false>), grid, block, 0, stream, x, x_stride, y, y_stride, n, c, d, table,
                       (A)sign, small);
  else
    hipLaunchKernelGGL((k_rope_apply<T, A, 2, true>), grid, block, 0, stream, x, x_stride, y, y_stride, n, c, d, table,
                       (A)sign, small);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // namespace rope
}  // namespace me

using namespace me;
using namespace me::rope;

extern "C" {

int me_rope_table(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *unit, int32_t d, double base,
                  int32_t table_f64, void *table_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(ncol >= 2 && ncol <= ME_MAX_DIM + 1, "coordinate size (D+1) must be in [2, 8]");
  const int D = ncol - 1;
  ME_CHECK(d >= 2 && d % 2 == 0, "the head size d must be even");
  const int P = d / 2;
  ME_CHECK(P >= D, "the head size d must hold one pair per spatial axis: d / 2 >= D");
  ME_CHECK(P <= kMaxPairs, "the head size d must not exceed 2 * ME_ROPE_MAX_PAIRS");
  ME_CHECK(std::isfinite(base) && base > 0.0, "base must be finite and greater than 0");
  ME_CHECK(unit != nullptr, "unit must hold one value per spatial axis");
  ME_CHECK(n >= 0 && n < (1ll << 31), "the row count must fit in int32");
  TableArgs args;
  memset(&args, 0, sizeof(args));
  for (int a = 0; a < D; ++a) {
    ME_CHECK(unit[a] >= 1, "every unit must be at least 1");
    args.unit[a] = (double)unit[a];
  }
  if (n == 0) return 0;
  ME_CHECK(coords_dev != nullptr && table_dev != nullptr, "coords and table must be given");
  ME_CHECK(aligned({table_dev}, 16), "the table must be 16-byte aligned");
  const int m = P / D;
  for (int j = 0; j < m; ++j) args.omega[j] = std::pow(base, -(double)j / (double)m);
  const dim3 grid(capped_grid(n * P)), block(256);
  if (table_f64)
    hipLaunchKernelGGL(k_rope_table<double>, grid, block, 0, stream, coords_dev, n, (int)ncol, P, m, args,
                       (double *)table_dev);
  else
    hipLaunchKernelGGL(k_rope_table<float>, grid, block, 0, stream, coords_dev, n, (int)ncol, P, m, args,
                       (float *)table_dev);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_rope_apply(const void *x_dev, int64_t x_stride, void *y_dev, int64_t y_stride, int64_t n, int32_t heads, int32_t d,
                  const void *table_dev, int32_t sign, int32_t dtype, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(d >= 2 && d % 2 == 0, "the head size d must be even");
  ME_CHECK(d / 2 <= kMaxPairs, "the head size d must not exceed 2 * ME_ROPE_MAX_PAIRS");
  ME_CHECK(heads >= 1 && (int64_t)heads * d < (1ll << 31), "heads must be at least 1 and heads * d must fit in int32");
  ME_CHECK(sign == 1 || sign == -1, "sign must be +1 or -1");
  ME_CHECK(dtype == ME_ROPE_F32 || dtype == ME_ROPE_BF16 || dtype == ME_ROPE_F64,
           "dtype must be ME_ROPE_F32, ME_ROPE_BF16 or ME_ROPE_F64");
  const int c = heads * d;
  ME_CHECK(x_stride >= c && y_stride >= c, "a row stride must be at least heads * d");
  ME_CHECK(n >= 0 && n < (1ll << 31), "the row count must fit in int32");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && y_dev != nullptr && table_dev != nullptr, "x, y and table must be given");
  const int elem = dtype == ME_ROPE_BF16 ? 2 : dtype == ME_ROPE_F32 ? 4 : 8;
  ME_CHECK(aligned({x_dev, y_dev}, elem) && aligned({table_dev}, 16),
           "x and y must be aligned to their element, the table to 16 bytes");
  if (dtype == ME_ROPE_F32)
    return apply<float, float>((const float *)x_dev, x_stride, (float *)y_dev, y_stride, n, c, d, (const float *)table_dev,
                               sign, stream);
  if (dtype == ME_ROPE_BF16)
    return apply<__bf16, float>((const __bf16 *)x_dev, x_stride, (__bf16 *)y_dev, y_stride, n, c, d,
                                (const float *)table_dev, sign, stream);
  return apply<double, double>((const double *)x_dev, x_stride, (double *)y_dev, y_stride, n, c, d,
                               (const double *)table_dev, sign, stream);
}

}  // extern "C"
