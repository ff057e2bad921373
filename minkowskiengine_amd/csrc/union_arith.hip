// Arithmetic between two sparse tensors on different coordinate maps for gfx950 (MI355X): out = a (op) b on the union of
// the two maps, op in {+, -, *, /} (reference: MinkowskiTensor._binary_functor, MinkowskiTensor.py:511-546).
//
// The reference zero-fills the output, writes a's rows into it through an index, reads b's union rows back out of it,
// applies the operator and writes them through the index again: about five passes over the output in four indexed
// launches.  Here every union row is produced once:
//   * two row tables a_of_u / b_of_u (int32 [Nu], -1 = the input has no such row) say where a union row comes from; they
//     and their inverses u_of_a / u_of_b are built once per pair of maps by k_tables from what union_map returns;
//   * k_union_fw: a lane owns (union row, 16-byte piece).  Both table entries are loaded first, then both input pieces
//     unconditionally through the clamped index, the value masked afterwards (docs/HISTORY.md 10.5: no branch round a
//     load); the piece is stored once with one vector store.  No zero fill, no atomics, no dependence on the launch
//     geometry: bitwise reproducible.  The lanes of a row ask for the same table entry, which the memory pipe serves as
//     one request per wave: the tables cost 8 bytes per row, not per element;
//   * semantics are the reference's as it behaves: fn(a, b) where both hold the row, `a` unchanged where only a holds it
//     (for * and / as well), fn(0, b) where only b holds it;
//   * k_union_bw_a / k_union_bw_b: every input row has exactly one union row, so a gradient row is a gather of dOut times
//     the local derivative; nothing is reduced, nothing to order.  One launch per wanted gradient.
// bf16 rows are widened to fp32, combined there and rounded once at the store.
#include "piece.hpp"

namespace me {
namespace uarith {

// ---- row tables ----------------------------------------------------------------------------------------------------------
// thread i < na: row i of a; else row i - na of b.  The inverse tables are filled with -1 before (hipMemsetAsync 0xff);
// coordinates are unique within a map, so no two threads write one slot of the same table.  A union row outside [0, nu)
// is recorded as -1 in u_of_* and not scattered: a later pass then treats the row as absent instead of reading outside.
__global__ __launch_bounds__(256) void k_tables(const int64_t *__restrict__ a_union, int64_t na,
                                               const int64_t *__restrict__ b_union, int64_t nb, int64_t nu,
                                               int32_t *__restrict__ u_of_a, int32_t *__restrict__ u_of_b,
                                               int32_t *__restrict__ a_of_u, int32_t *__restrict__ b_of_u) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= na + nb) return;
  const bool is_a = i < na;
  const int64_t r = is_a ? i : i - na;
  const int64_t u = is_a ? a_union[r] : b_union[r];
  const bool ok = u >= 0 && u < nu;
  (is_a ? u_of_a : u_of_b)[r] = ok ? (int32_t)u : -1;
  if (ok) (is_a ? a_of_u : b_of_u)[u] = (int32_t)r;
}

template <int OP, typename A>
__device__ __forceinline__ A apply(A x, A y) {
  if constexpr (OP == ME_UNION_ADD) return x + y;
  else if constexpr (OP == ME_UNION_SUB) return x - y;
  else if constexpr (OP == ME_UNION_MUL) return x * y;
  else return x / y;
}

// ---- forward -------------------------------------------------------------------------------------------------------------
// Byte model: (Na + Nb + Nu) * C * sizeof(T) + 8 * Nu.  a / b are never null here (the launcher substitutes the other
// operand for an input without rows: every value read through it is masked).
template <typename T, typename A, int V, int OP>
__global__ __launch_bounds__(256) void k_union_fw(const T *__restrict__ a, const T *__restrict__ b, int c,
                                                 const int32_t *__restrict__ a_of_u, const int32_t *__restrict__ b_of_u,
                                                 int64_t na, int64_t nb, int64_t nu, T *__restrict__ out) {
  const int pieces = c / V;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nu * pieces) return;
  const int64_t u = idx / pieces;
  const int ch = (int)(idx % pieces) * V;
  const int32_t ia = a_of_u[u], ib = b_of_u[u];
  const bool ha = ia >= 0 && ia < na, hb = ib >= 0 && ib < nb;
  const Piece<V, T> av = load_piece<T, V, T>(a + (int64_t)(ha ? ia : 0) * c + ch);
  const Piece<V, T> bv = load_piece<T, V, T>(b + (int64_t)(hb ? ib : 0) * c + ch);
  Piece<V, T> o;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const T x = ha ? av.v[j] : (T)0;
    o.v[j] = hb ? (T)apply<OP, A>((A)x, (A)bv.v[j]) : x;
  }
  store_piece<T, V, T>(out + u * c + ch, o);
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// grad_a[i] = dOut[u] * d fn(a, b) / d a on a shared row (1, 1, b, 1 / b), dOut[u] on a row only a holds.
// Byte model: 2 * Na * C * sizeof(T) + 8 * Na (+ Na * C * sizeof(T) for * and /, which read b).
template <typename T, typename A, int V, int OP>
__global__ __launch_bounds__(256) void k_union_bw_a(const T *__restrict__ g, const T *__restrict__ b, int c,
                                                   const int32_t *__restrict__ u_of_a, const int32_t *__restrict__ b_of_u,
                                                   int64_t na, int64_t nb, int64_t nu, T *__restrict__ ga) {
  const int pieces = c / V;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= na * pieces) return;
  const int64_t i = idx / pieces;
  const int ch = (int)(idx % pieces) * V;
  const int32_t u = u_of_a[i];
  const bool hu = u >= 0 && u < nu;
  const Piece<V, T> gv = load_piece<T, V, T>(g + (int64_t)(hu ? u : 0) * c + ch);
  Piece<V, T> o;
  if constexpr (OP == ME_UNION_ADD || OP == ME_UNION_SUB) {
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = hu ? gv.v[j] : (T)0;
  } else {
    const int32_t ib = b_of_u[hu ? u : 0];
    const bool hb = hu && ib >= 0 && ib < nb;
    const Piece<V, T> bv = load_piece<T, V, T>(b + (int64_t)(hb ? ib : 0) * c + ch);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const T gj = hu ? gv.v[j] : (T)0;
      o.v[j] = hb ? (T)apply<OP, A>((A)gj, (A)bv.v[j]) : gj;     // g * b, g / b
    }
  }
  store_piece<T, V, T>(ga + i * c + ch, o);
}

// grad_b[j] = dOut[u] * d fn(x, b) / d b with x = a's row, or 0 where a has none: g, -g, g * x, -g * ((x / b) / b) (the
// order of torch's own division gradient).  Byte model: 2 * Nb * C * sizeof(T) + 8 * Nb (+ a for * and /, + b for /).
template <typename T, typename A, int V, int OP>
__global__ __launch_bounds__(256) void k_union_bw_b(const T *__restrict__ g, const T *__restrict__ a, const T *__restrict__ b,
                                                   int c, const int32_t *__restrict__ u_of_b,
                                                   const int32_t *__restrict__ a_of_u, int64_t na, int64_t nb, int64_t nu,
                                                   T *__restrict__ gb) {
  const int pieces = c / V;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nb * pieces) return;
  const int64_t i = idx / pieces;
  const int ch = (int)(idx % pieces) * V;
  const int32_t u = u_of_b[i];
  const bool hu = u >= 0 && u < nu;
  const Piece<V, T> gv = load_piece<T, V, T>(g + (int64_t)(hu ? u : 0) * c + ch);
  Piece<V, T> o;
  if constexpr (OP == ME_UNION_ADD) {
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = hu ? gv.v[j] : (T)0;
  } else if constexpr (OP == ME_UNION_SUB) {
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = hu ? (T)(-(A)gv.v[j]) : (T)0;
  } else {
    const int32_t ia = a_of_u[hu ? u : 0];
    const bool ha = hu && ia >= 0 && ia < na;
    const Piece<V, T> av = load_piece<T, V, T>(a + (int64_t)(ha ? ia : 0) * c + ch);
    Piece<V, T> bv;
    if constexpr (OP == ME_UNION_DIV) bv = load_piece<T, V, T>(b + i * c + ch);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const A gj = hu ? (A)gv.v[j] : (A)0, x = ha ? (A)av.v[j] : (A)0;
      if constexpr (OP == ME_UNION_MUL) {
        o.v[j] = (T)(gj * x);
      } else {
        const A y = (A)bv.v[j];
        o.v[j] = (T)(-gj * ((x / y) / y));
      }
    }
  }
  store_piece<T, V, T>(gb + i * c + ch, o);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
#define ME_UARITH_OP(op, ...)                                                                    \
  switch (op) {                                                                                  \
    case ME_UNION_ADD: { constexpr int OP = ME_UNION_ADD; __VA_ARGS__; break; }                  \
    case ME_UNION_SUB: { constexpr int OP = ME_UNION_SUB; __VA_ARGS__; break; }                  \
    case ME_UNION_MUL: { constexpr int OP = ME_UNION_MUL; __VA_ARGS__; break; }                  \
    case ME_UNION_DIV: { constexpr int OP = ME_UNION_DIV; __VA_ARGS__; break; }                  \
    default: ME_FAIL("op must be ME_UNION_ADD, _SUB, _MUL or _DIV");                             \
  }

inline int check_sizes(int32_t c, int64_t na, int64_t nb, int64_t nu, int32_t op) {
  ME_CHECK(c > 0, "invalid channel count");
  ME_CHECK(na >= 0 && nb >= 0 && nu >= 0 && na < (1ll << 31) && nb < (1ll << 31) && nu < (1ll << 31),
           "row counts must fit in int32");
  ME_CHECK(nu <= na + nb, "the union cannot have more rows than both inputs together");
  ME_CHECK(op >= ME_UNION_ADD && op <= ME_UNION_DIV, "op must be ME_UNION_ADD, _SUB, _MUL or _DIV");
  return 0;
}

template <typename T, typename A>
int forward(const T *a, const T *b, int32_t c, const int32_t *a_of_u, const int32_t *b_of_u, int64_t na, int64_t nb,
            int64_t nu, int32_t op, T *out, hipStream_t stream) {
  if (int rc = check_sizes(c, na, nb, nu, op)) return rc;
  if (nu == 0) return 0;
  ME_CHECK(a_of_u != nullptr && b_of_u != nullptr && out != nullptr, "the row tables and out must be given");
  ME_CHECK((na == 0 || a != nullptr) && (nb == 0 || b != nullptr), "a and b must be given");
  // an input without rows is never selected: any readable row stands in for it (nu > 0, so the other one has rows)
  if (na == 0) a = b;
  if (nb == 0) b = a;
  const int v = piece_width<T>(kPieceHalf, c, {a, b, out});
  const int64_t total = nu * (c / v);
  ME_CHECK(ceil_div(total, 256) < (1ll << 31), "Nu * C too large for one launch");
  const dim3 grid((unsigned)ceil_div(total, 256)), block(256);
  ME_UARITH_OP(op, ME_PIECE_DISPATCH(T, kPieceHalf, v,
                                     hipLaunchKernelGGL((k_union_fw<T, A, V, OP>), grid, block, 0, stream, a, b, c, a_of_u,
                                                        b_of_u, na, nb, nu, out)));
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, typename A>
int backward(const T *g, const T *a, const T *b, int32_t c, const int32_t *u_of_a, const int32_t *u_of_b,
             const int32_t *a_of_u, const int32_t *b_of_u, int64_t na, int64_t nb, int64_t nu, int32_t op, T *ga, T *gb,
             hipStream_t stream) {
  if (int rc = check_sizes(c, na, nb, nu, op)) return rc;
  const bool mul_div = op == ME_UNION_MUL || op == ME_UNION_DIV;
  ME_CHECK(nu == 0 || g != nullptr, "grad_out must be given");
  if (ga != nullptr && na > 0) {
    ME_CHECK(nu > 0 && u_of_a != nullptr, "u_of_a must be given");
    ME_CHECK(!mul_div || (b_of_u != nullptr && (nb == 0 || b != nullptr)), "b and b_of_u must be given for * and /");
    const T *bb = (mul_div && nb > 0) ? b : g;       // nb == 0: never selected
    const int v = piece_width<T>(kPieceHalf, c, {g, bb, ga});
    const int64_t total = na * (c / v);
    ME_CHECK(ceil_div(total, 256) < (1ll << 31), "Na * C too large for one launch");
    const dim3 grid((unsigned)ceil_div(total, 256)), block(256);
    ME_UARITH_OP(op, ME_PIECE_DISPATCH(T, kPieceHalf, v,
                                       hipLaunchKernelGGL((k_union_bw_a<T, A, V, OP>), grid, block, 0, stream, g, bb, c,
                                                          u_of_a, b_of_u, na, nb, nu, ga)));
    ME_LAUNCH_CHECK();
  }
  if (gb != nullptr && nb > 0) {
    ME_CHECK(nu > 0 && u_of_b != nullptr, "u_of_b must be given");
    ME_CHECK(!mul_div || (a_of_u != nullptr && (na == 0 || a != nullptr)), "a and a_of_u must be given for * and /");
    ME_CHECK(op != ME_UNION_DIV || b != nullptr, "b must be given for /");
    const T *aa = (mul_div && na > 0) ? a : g;       // na == 0: never selected
    const T *bb = op == ME_UNION_DIV ? b : g;
    const int v = piece_width<T>(kPieceHalf, c, {g, aa, bb, gb});
    const int64_t total = nb * (c / v);
    ME_CHECK(ceil_div(total, 256) < (1ll << 31), "Nb * C too large for one launch");
    const dim3 grid((unsigned)ceil_div(total, 256)), block(256);
    ME_UARITH_OP(op, ME_PIECE_DISPATCH(T, kPieceHalf, v,
                                       hipLaunchKernelGGL((k_union_bw_b<T, A, V, OP>), grid, block, 0, stream, g, aa, bb,
                                                          c, u_of_b, a_of_u, na, nb, nu, gb)));
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace uarith
}  // namespace me

using namespace me;
using namespace me::uarith;

extern "C" {

int me_union_tables(const int64_t *a_union, int64_t na, const int64_t *b_union, int64_t nb, int64_t nu, int32_t *u_of_a,
                    int32_t *u_of_b, int32_t *a_of_u, int32_t *b_of_u, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(na >= 0 && nb >= 0 && nu >= 0 && na < (1ll << 31) && nb < (1ll << 31) && nu < (1ll << 31),
           "row counts must fit in int32");
  ME_CHECK((na == 0 || (a_union != nullptr && u_of_a != nullptr)) && (nb == 0 || (b_union != nullptr && u_of_b != nullptr)),
           "the union rows of both inputs and their int32 copies must be given");
  ME_CHECK(nu == 0 || (a_of_u != nullptr && b_of_u != nullptr), "a_of_u and b_of_u must be given");
  if (nu > 0) {
    ME_HIP(hipMemsetAsync(a_of_u, 0xff, (size_t)nu * 4, stream));
    ME_HIP(hipMemsetAsync(b_of_u, 0xff, (size_t)nu * 4, stream));
  }
  if (na + nb == 0) return 0;
  hipLaunchKernelGGL(k_tables, dim3((unsigned)ceil_div(na + nb, 256)), dim3(256), 0, stream, a_union, na, b_union, nb, nu,
                     u_of_a, u_of_b, a_of_u, b_of_u);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_union_arith_f32(const float *a, const float *b, int32_t c, const int32_t *a_of_u, const int32_t *b_of_u, int64_t na,
                       int64_t nb, int64_t nu, int32_t op, float *out, void *stream) {
  return forward<float, float>(a, b, c, a_of_u, b_of_u, na, nb, nu, op, out, (hipStream_t)stream);
}
int me_union_arith_bf16(const uint16_t *a, const uint16_t *b, int32_t c, const int32_t *a_of_u, const int32_t *b_of_u,
                        int64_t na, int64_t nb, int64_t nu, int32_t op, uint16_t *out, void *stream) {
  return forward<__bf16, float>((const __bf16 *)a, (const __bf16 *)b, c, a_of_u, b_of_u, na, nb, nu, op, (__bf16 *)out,
                                (hipStream_t)stream);
}
int me_union_arith_f64(const double *a, const double *b, int32_t c, const int32_t *a_of_u, const int32_t *b_of_u, int64_t na,
                       int64_t nb, int64_t nu, int32_t op, double *out, void *stream) {
  return forward<double, double>(a, b, c, a_of_u, b_of_u, na, nb, nu, op, out, (hipStream_t)stream);
}

int me_union_arith_backward_f32(const float *grad_out, const float *a, const float *b, int32_t c, const int32_t *u_of_a,
                                const int32_t *u_of_b, const int32_t *a_of_u, const int32_t *b_of_u, int64_t na, int64_t nb,
                                int64_t nu, int32_t op, float *grad_a, float *grad_b, void *stream) {
  return backward<float, float>(grad_out, a, b, c, u_of_a, u_of_b, a_of_u, b_of_u, na, nb, nu, op, grad_a, grad_b,
                                (hipStream_t)stream);
}
int me_union_arith_backward_bf16(const uint16_t *grad_out, const uint16_t *a, const uint16_t *b, int32_t c,
                                 const int32_t *u_of_a, const int32_t *u_of_b, const int32_t *a_of_u, const int32_t *b_of_u,
                                 int64_t na, int64_t nb, int64_t nu, int32_t op, uint16_t *grad_a, uint16_t *grad_b,
                                 void *stream) {
  return backward<__bf16, float>((const __bf16 *)grad_out, (const __bf16 *)a, (const __bf16 *)b, c, u_of_a, u_of_b, a_of_u,
                                 b_of_u, na, nb, nu, op, (__bf16 *)grad_a, (__bf16 *)grad_b, (hipStream_t)stream);
}
int me_union_arith_backward_f64(const double *grad_out, const double *a, const double *b, int32_t c, const int32_t *u_of_a,
                                const int32_t *u_of_b, const int32_t *a_of_u, const int32_t *b_of_u, int64_t na, int64_t nb,
                                int64_t nu, int32_t op, double *grad_a, double *grad_b, void *stream) {
  return backward<double, double>(grad_out, a, b, c, u_of_a, u_of_b, a_of_u, b_of_u, na, nb, nu, op, grad_a, grad_b,
                                  (hipStream_t)stream);
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_union_arith(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::uarith::k_tables));
}
