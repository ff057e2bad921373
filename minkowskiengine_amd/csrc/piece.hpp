// The row piece of the element-wise, gather and normalisation kernels: V consecutive channels of one row [n, c], moved
// with one vector access and held in an accumulation type.  Device side: the piece and its loads and stores.  Host side:
// the alignment test, the three rules that choose V, the dispatch over V and the grid of a kernel whose threads own one
// (row, piece) each.
#pragma once
#include "common.hpp"

#include <initializer_list>

namespace me {

// V consecutive channels of one row in A, whatever the storage type T: fp32 for float and __bf16 rows (bf16 features are
// summed / compared in fp32 and rounded once at the store, like the convolution kernels), double for float64 sums, T
// itself for a plain copy (also of int32 / int64 indices).  One access of V * sizeof(T) bytes: 16 bytes for (float, 4),
// (__bf16, 8) and (double, 2), 8 bytes for (float, 2) and (__bf16, 4), one element for V = 1.
template <int V, typename A = float>
struct Piece {
  A v[V];
};
template <typename T, int V, typename A = float>
__device__ __forceinline__ Piece<V, A> load_piece(const T *p) {
  Piece<V, A> r;
  if constexpr (V == 1) {
    r.v[0] = (A)*p;
  } else {
    typedef T tvec __attribute__((ext_vector_type(V)));
    const tvec t = *reinterpret_cast<const tvec *>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = (A)t[j];
  }
  return r;
}
template <typename T, int V, typename A = float>
__device__ __forceinline__ void store_piece(T *p, const Piece<V, A> &r) {
  if constexpr (V == 1) {
    *p = (T)r.v[0];
  } else {
    typedef T tvec __attribute__((ext_vector_type(V)));
    tvec t;
#pragma unroll
    for (int j = 0; j < V; ++j) t[j] = (T)r.v[j];
    *reinterpret_cast<tvec *>(p) = t;
  }
}

// V consecutive fp32 values (weights, bias, statistics of the channels of a piece): 16-byte loads when V is a multiple
// of 4 — the host checks the alignment
template <int V>
__device__ __forceinline__ void load_f32(const float *__restrict__ p, float (&v)[V]) {
  if constexpr (V % 4 == 0) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
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

// rows of chunk g of n rows split into G chunks: [g * n / G, (g + 1) * n / G)
__device__ __forceinline__ int64_t chunk_begin(int64_t g, int64_t n, int64_t G) { return g * n / G; }

// ---- host side ------------------------------------------------------------------------------------------------------
// every pointer a multiple of `bytes` (NULL, an operand that is not given, is skipped)
inline bool aligned(std::initializer_list<const void *> ptrs, uintptr_t bytes) {
  for (const void *p : ptrs)
    if (p != nullptr && (uintptr_t)p % bytes != 0) return false;
  return true;
}
// the alignment the width rules ask about: 16, 8 or 1
inline int common_alignment(std::initializer_list<const void *> ptrs) {
  return aligned(ptrs, 16) ? 16 : aligned(ptrs, 8) ? 8 : 1;
}

// The widest piece for rows of c channels of e-byte elements whose addresses share `align`.  Every rule takes 16 bytes
// (W = 16 / e channels) when c % W == 0 at 16-byte alignment and falls back to one channel; they differ in the one
// width between (tests pin each: the kernels of a family exist for exactly these widths).
enum PieceRule {
  kPieceHalf,      // 8 bytes at 8-byte alignment: 2 fp32, 4 bf16, none for float64 (gathers, union arithmetic, direct max)
  kPieceBf16Half,  // 8 bytes at 8-byte alignment for bf16 only (local pooling, broadcast, channelwise forward)
  kPieceNorm,      // 4 channels at 16-byte alignment: bf16 rows of 4, 12, 20, ... channels (the normalisations)
};
// the middle width of a rule (1: it has none)
constexpr int piece_mid(int e, PieceRule rule) {
  return rule == kPieceHalf ? 8 / e : rule == kPieceBf16Half ? (e == 2 ? 4 : 1) : (16 / e > 4 ? 4 : 1);
}
constexpr int piece_width(int e, int c, int align, PieceRule rule) {
  const int W = 16 / e, M = piece_mid(e, rule);
  if (c % W == 0 && align % 16 == 0) return W;
  if (M > 1 && c % M == 0 && align % (rule == kPieceNorm ? 16 : 8) == 0) return M;
  return 1;
}
template <typename T>
inline int piece_width(PieceRule rule, int c, std::initializer_list<const void *> ptrs) {
  return piece_width((int)sizeof(T), c, common_alignment(ptrs), rule);
}

// (element bytes, c, alignment) -> width by kPieceHalf, kPieceBf16Half, kPieceNorm
#define ME_PIECE_IS(e, c, align, half, bf16_half, norm)                                                          \
  static_assert(piece_width(e, c, align, kPieceHalf) == half && piece_width(e, c, align, kPieceBf16Half) == bf16_half && \
                piece_width(e, c, align, kPieceNorm) == norm, "piece width rule")
ME_PIECE_IS(4, 96, 16, 4, 4, 4);
ME_PIECE_IS(4, 96, 8, 2, 1, 1);
ME_PIECE_IS(4, 6, 16, 2, 1, 1);
ME_PIECE_IS(4, 6, 8, 2, 1, 1);
ME_PIECE_IS(4, 96, 4, 1, 1, 1);
ME_PIECE_IS(4, 7, 16, 1, 1, 1);
ME_PIECE_IS(2, 96, 16, 8, 8, 8);
ME_PIECE_IS(2, 12, 16, 4, 4, 4);
ME_PIECE_IS(2, 12, 8, 4, 4, 1);
ME_PIECE_IS(2, 96, 8, 4, 4, 1);
ME_PIECE_IS(2, 96, 4, 1, 1, 1);
ME_PIECE_IS(2, 7, 16, 1, 1, 1);
#undef ME_PIECE_IS
// float64 rows take kPieceHalf only
static_assert(piece_width(8, 4, 16, kPieceHalf) == 2, "piece width rule");
static_assert(piece_width(8, 4, 8, kPieceHalf) == 1, "piece width rule");
static_assert(piece_width(8, 3, 16, kPieceHalf) == 1, "piece width rule");

// `...` with constexpr int V = v, instantiated for exactly the widths that `rule` can return for T: 16 / sizeof(T), the
// rule's middle width where it has one, and 1
#define ME_PIECE_DISPATCH(T, rule, v, ...)                                                         \
  do {                                                                                             \
    constexpr int W_ = 16 / (int)sizeof(T), M_ = ::me::piece_mid((int)sizeof(T), ::me::rule);      \
    if ((v) == W_) { constexpr int V = W_; __VA_ARGS__; }                                          \
    else if ((v) == M_) { constexpr int V = M_; __VA_ARGS__; }                                     \
    else { constexpr int V = 1; __VA_ARGS__; }                                                     \
  } while (0)

// workgroups of 256 threads that own one (row, piece of v channels) each
inline dim3 piece_grid(int64_t rows, int c, int v) { return dim3((unsigned)ceil_div(rows * (c / v), 256)); }

}  // namespace me
