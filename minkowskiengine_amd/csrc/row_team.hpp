// The row team of the row-norm kernels (layer_norm.hip, ada_layer_norm.hip): a row [c] lives in the registers of a team of
// L lanes (L = 1 .. 64, a power of two), P pieces of V channels per lane; piece q = p * L + lane holds the channels
// [q V, q V + V).  Device side: the exchanges inside a team, the ONE balanced tree of every row sum, the centring both
// passes share, the rounded-once rsqrt, the channels and parameters of a lane.  Host side: the (L, P) dispatch.  Both
// files form xhat with these helpers alone, so they give the same bits for the same row.
#pragma once
#include "piece.hpp"

#include <type_traits>

// every product and sum below rounds on its own, in every instantiation alike; the fused multiply-adds are written out
// (the pragma holds to the end of the including file)
#pragma clang fp contract(off)

namespace me {
namespace lnorm {

constexpr int kThreads = 256;
constexpr int kMaxC = ME_LNORM_MAX_C;
constexpr int kMaxChunks = 1024;       // records of the backward: 256 CUs x 4 workgroups
constexpr int kChunkBytes = 16384;     // a chunk holds at least this much of x
constexpr int kMaxBlocks = 2048;       // forward: 256 CUs x 8 workgroups, the rest is the row loop

// v of lane (lane ^ OFF): a swizzle inside 32 lanes, a permute across the halves of the wave
template <int OFF>
__device__ __forceinline__ float lane_xor(float v) {
  if constexpr (OFF < 32)
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (OFF << 10) | 0x1f));
  else
    return __shfl_xor(v, 32, 64);
}

// sum of v[0 .. N) as a balanced tree: blocks of 2, 4, .. N consecutive values
template <int N>
__device__ __forceinline__ float tree_sum(float (&v)[N]) {
#pragma unroll
  for (int s = 1; s < N; s <<= 1)
#pragma unroll
    for (int j = 0; j < N; j += 2 * s) v[j] += v[j + s];
  return v[0];
}

template <int OFF, int N>
__device__ __forceinline__ void xor_add(float (&s)[N]) {
#pragma unroll
  for (int p = 0; p < N; ++p) s[p] += lane_xor<OFF>(s[p]);
}
// s[p] summed over the lanes whose index differs in the bits [LO, HI): every lane ends with the same values
template <int LO, int HI, int N>
__device__ __forceinline__ void xor_reduce(float (&s)[N]) {
  if constexpr (LO <= 1 && 1 < HI) xor_add<1>(s);
  if constexpr (LO <= 2 && 2 < HI) xor_add<2>(s);
  if constexpr (LO <= 4 && 4 < HI) xor_add<4>(s);
  if constexpr (LO <= 8 && 8 < HI) xor_add<8>(s);
  if constexpr (LO <= 16 && 16 < HI) xor_add<16>(s);
  if constexpr (LO <= 32 && 32 < HI) xor_add<32>(s);
}

// the sum of a[p][v] over the row of the team (destroys a)
template <int L, int P, int V>
__device__ __forceinline__ float team_sum(float (&a)[P][V]) {
  float s[P];
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = tree_sum<V>(a[p]);
  xor_reduce<1, L>(s);
  return tree_sum<P>(s);
}

// 1 / sqrt(v) rounded once: the quotient of the two correctly rounded operations can be an ulp off, and the backward pass
// multiplies that error by 1 / (1 - xhat^2) where one channel carries a row.  One Newton step on the exact residual
// 1 - v r^2 (the rounding of r * r is recovered by an fma); a residual that is not finite (v = inf) keeps r
__device__ __forceinline__ float rsqrt_rn(float v) {
  const float r = 1.f / sqrtf(v);
  const float p = r * r, pe = __builtin_fmaf(r, r, -p);
  const float e = __builtin_fmaf(-v, pe, __builtin_fmaf(-v, p, 1.f));
  return __builtin_isfinite(e) ? __builtin_fmaf(0.5f * r, e, r) : r;
}

// d = the row minus its mean, as BOTH passes compute it (same bits): x[0] of the row sits in the first lane of the team;
// layer norm does not change when a row is shifted by it, the differences of close values are exact, and a constant row
// is centred to exactly 0.  xv: the row with zeros past it; tmp: scratch.  -> the mean (x[0] + the mean of the differences)
template <int L, int P, int V>
__device__ __forceinline__ float centre(const float (&xv)[P][V], const bool (&ok)[P], float fc, float (&d)[P][V],
                                        float (&tmp)[P][V]) {
  const float x0 = __shfl(xv[0][0], (int)(threadIdx.x & 63) & ~(L - 1), 64);
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < V; ++j) tmp[p][j] = d[p][j] = ok[p] ? xv[p][j] - x0 : 0.f;
  const float dm = team_sum<L, P, V>(tmp) / fc;
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < V; ++j) d[p][j] = ok[p] ? d[p][j] - dm : 0.f;
  return x0 + dm;
}

// the channels of a lane: ch[p] of piece p (0 for a piece past the row), ok[p] whether the piece is inside the row
template <int V, int L, int P>
__device__ __forceinline__ void lane_pieces(int c, int (&ch)[P], bool (&ok)[P]) {
  const int tl = threadIdx.x % L, pieces = c / V;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int q = p * L + tl;
    ok[p] = q < pieces;
    ch[p] = ok[p] ? q * V : 0;
  }
}
template <int V, int P>
__device__ __forceinline__ void load_param(const float *w, const int (&ch)[P], float fill, float (&out)[P][V]) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (w != nullptr) {
      load_f32<V>(w + ch[p], out[p]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) out[p][j] = fill;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline int64_t gcd(int64_t a, int64_t b) {
  while (b != 0) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// f(L, P) with both as compile-time constants, for the team that serves `pieces` pieces of V channels: the smallest
// power of two L <= 64 that covers them with P = 1, else L = 64 and the smallest power of two P
template <int V, typename F>
inline void for_team(int pieces, F &&f) {
  int L = 1, P = 1;
  while (L < kWave && L < pieces) L <<= 1;
  while (L * P < pieces) P <<= 1;
#define ME_LN_TEAM(l, p)                                                                        \
  if (L == l && P == p) {                                                                       \
    if constexpr (p * V * kWave <= kMaxC) f(std::integral_constant<int, l>{}, std::integral_constant<int, p>{}); \
    return;                                                                                     \
  }
  ME_LN_TEAM(1, 1) ME_LN_TEAM(2, 1) ME_LN_TEAM(4, 1) ME_LN_TEAM(8, 1) ME_LN_TEAM(16, 1) ME_LN_TEAM(32, 1)
  ME_LN_TEAM(64, 1) ME_LN_TEAM(64, 2) ME_LN_TEAM(64, 4) ME_LN_TEAM(64, 8) ME_LN_TEAM(64, 16) ME_LN_TEAM(64, 32)
#undef ME_LN_TEAM
}

}  // namespace lnorm
}  // namespace me
