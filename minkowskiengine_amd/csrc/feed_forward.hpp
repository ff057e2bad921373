// Fragment helpers of the fused MLP kernels for gfx950 (feed_forward.hip, gated_feed_forward.hip): the 32x32 MFMA shape of
// both dtypes, operand fragments and their loads from LDS, the accumulator-as-operand identity, the activations, the
// 16-byte staging of weight blocks and the weight transposition; then, host only, the one copy of the launch and policy code
// of both units, which each unit instantiates with a description of its family.
//
// One 32x32 MFMA shape serves both dtypes: v_mfma_f32_32x32x16_bf16 on bf16 rows, the exact v_mfma_f32_32x32x2_f32 on fp32
// rows; C/D lane map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The 16 accumulator registers of a
// tile are the two k-steps of the B operand of a following product with no lane movement: registers 8 s .. 8 s + 7 are
// k-step s, element j of lane half h being row 16 s + 8 (j >> 2) + 4 h + (j & 3); the A operand of that product is read in
// the same permuted k order (ffn_load44).
#pragma once
#include "common.hpp"

#include <algorithm>
#include <initializer_list>

namespace me {
namespace ffn {

typedef float ff_f32x16 __attribute__((ext_vector_type(16)));
typedef float ff_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ff_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ff_bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;            // four waves
constexpr int kRows = ME_FFN_ROWS;       // rows of a workgroup (step), 32 per wave
constexpr int kLdsBudget = 160 * 1024;
constexpr int kTargetGroups = 512;       // workgroups the weight-gradient grid aims for (two per CU)

template <typename T> struct FfnT;
template <> struct FfnT<__bf16> {
  typedef ff_bf16x8 vec;            // a 16-byte piece
  static constexpr int EPP = 8;     // elements of a 16-byte piece
  static constexpr int PAD = 8;     // LDS rows: + 16 bytes
};
template <> struct FfnT<float> {
  typedef ff_f32x4 vec;
  static constexpr int EPP = 4;
  static constexpr int PAD = 4;
};

// 8 k-values of one operand row (lane half h of a 16-wide k-step; eight 32x32x2 steps on fp32 rows)
template <typename T> struct Frag;
template <> struct Frag<__bf16> { ff_bf16x8 v; };
template <> struct Frag<float> { float v[8]; };

__device__ __forceinline__ void ffn_mma(ff_f32x16 &acc, const Frag<__bf16> &a, const Frag<__bf16> &b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void ffn_mma(ff_f32x16 &acc, const Frag<float> &a, const Frag<float> &b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// 8 consecutive elements at p (16-byte aligned)
__device__ __forceinline__ Frag<__bf16> ffn_load8(const __bf16 *p) {
  Frag<__bf16> f;
  f.v = *reinterpret_cast<const ff_bf16x8 *>(p);
  return f;
}
__device__ __forceinline__ Frag<float> ffn_load8(const float *p) {
  Frag<float> f;
  const ff_f32x4 a = *reinterpret_cast<const ff_f32x4 *>(p), b = *reinterpret_cast<const ff_f32x4 *>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
// elements 0..3 at p, 4..7 at p + 8: the k order of an accumulator used as an operand
__device__ __forceinline__ Frag<__bf16> ffn_load44(const __bf16 *p) {
  Frag<__bf16> f;
  const ff_bf16x4 a = *reinterpret_cast<const ff_bf16x4 *>(p), b = *reinterpret_cast<const ff_bf16x4 *>(p + 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
__device__ __forceinline__ Frag<float> ffn_load44(const float *p) {
  Frag<float> f;
  const ff_f32x4 a = *reinterpret_cast<const ff_f32x4 *>(p), b = *reinterpret_cast<const ff_f32x4 *>(p + 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
// registers 8 s .. 8 s + 7 of a 32x32 tile as the fragment of k-step s (the one rounding of the hidden activation)
template <typename T> __device__ __forceinline__ Frag<T> ffn_acc_frag(const float (&x)[16], int s) {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = (T)x[8 * s + j];
  return f;
}
template <typename T> __device__ __forceinline__ Frag<T> ffn_zero_frag() {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = (T)0.f;
  return f;
}
// row of register reg of a 32x32 C/D tile in lane half h
__device__ __forceinline__ int ffn_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ void ffn_zero(ff_f32x16 &a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

// 4 consecutive channels of one row
__device__ __forceinline__ void ffn_store4(__bf16 *p, float a, float b, float c, float d) {
  ff_bf16x4 v;
  v[0] = (__bf16)a; v[1] = (__bf16)b; v[2] = (__bf16)c; v[3] = (__bf16)d;
  *reinterpret_cast<ff_bf16x4 *>(p) = v;
}
__device__ __forceinline__ void ffn_store4(float *p, float a, float b, float c, float d) {
  ff_f32x4 v;
  v[0] = a; v[1] = b; v[2] = c; v[3] = d;
  *reinterpret_cast<ff_f32x4 *>(p) = v;
}

// ---- activations, in fp32 --------------------------------------------------------------------------------------------
template <int A> __device__ __forceinline__ float act_f(float v) {
  if constexpr (A == ME_FFN_RELU) return v > 0.f ? v : 0.f;
  else if constexpr (A == ME_FFN_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  else if constexpr (A == ME_FFN_GELU_TANH) {
    const float u = 0.79788456080286536f * (v + 0.044715f * v * v * v);
    return 0.5f * v * (1.f + tanhf(u));
  } else return v / (1.f + expf(-v));
}
template <int A> __device__ __forceinline__ float act_g(float v) {
  if constexpr (A == ME_FFN_RELU) return v > 0.f ? 1.f : 0.f;   // act'(0) = 0, as in torch
  else if constexpr (A == ME_FFN_GELU)
    return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
  else if constexpr (A == ME_FFN_GELU_TANH) {
    const float t = tanhf(0.79788456080286536f * (v + 0.044715f * v * v * v));
    return 0.5f * (1.f + t) + 0.5f * v * (1.f - t * t) * 0.79788456080286536f * (1.f + 3.f * 0.044715f * v * v);
  } else {
    const float s = 1.f / (1.f + expf(-v));
    return s * (1.f + v * (1.f - s));
  }
}

// rows x cols elements (cols a multiple of a piece) from src (row stride ld_src) into the LDS image dst (row stride ld_dst)
template <typename T>
__device__ __forceinline__ void stage(const T *__restrict__ src, int64_t ld_src, int rows, int cols, T *dst, int ld_dst) {
  constexpr int EPP = FfnT<T>::EPP;
  using vec = typename FfnT<T>::vec;
  const int ppr = cols / EPP;
  for (int p = threadIdx.x; p < rows * ppr; p += kThreads) {
    const int rr = p / ppr, pc = p - rr * ppr;
    *reinterpret_cast<vec *>(dst + rr * ld_dst + pc * EPP) =
        *reinterpret_cast<const vec *>(src + (int64_t)rr * ld_src + pc * EPP);
  }
}

// a wave's fragment of 8 channels of 32 rows into its transposed image [channel][row]
template <typename T> __device__ __forceinline__ void scatter_t(T *s_t, int ldt, int ch0, int r, const Frag<T> &f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) s_t[(ch0 + j) * ldt + r] = f.v[j];
}

// ---- dst [cols, rows] = src [rows, cols]^T; both dimensions multiples of 32 ------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void k_ffn_transpose(const T *__restrict__ src, T *__restrict__ dst, int rows,
                                                            int cols) {
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = src[(int64_t)(r0 + ty + 8 * i) * cols + c0 + tx];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[(int64_t)(c0 + ty + 8 * i) * rows + r0 + tx] = tile[tx][ty + 8 * i];
}

// ---- host side ----------------------------------------------------------------------------------------------------------
template <typename K> inline int allow_lds(K fn, int64_t lds) {
  if (lds > 48 * 1024)
    ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
  return 0;
}

template <typename T> int transpose(const T *src, T *dst, int rows, int cols, hipStream_t stream) {
  hipLaunchKernelGGL(k_ffn_transpose<T>, dim3((unsigned)(cols / 32), (unsigned)(rows / 32)), dim3(kThreads), 0, stream,
                     src, dst, rows, cols);
  ME_LAUNCH_CHECK();
  return 0;
}

inline bool aligned16(std::initializer_list<const void *> ps) {
  for (const void *p : ps)
    if (((uintptr_t)p & 15) != 0) return false;
  return true;
}

// ---- launch and policy code of both MLPs (host only: nothing below reaches a kernel) --------------------------------------
// A unit describes its family by a struct F:
//   NZ                      first-layer (weight, bias) pairs: 1 plain, 2 gated (gate, up)
//   kMaxBf16, kMaxF32       the widest rows it instantiates kernels for
//   Rows<T>, Weights<T>     the argument structs of its row-stationary and weight-gradient kernels
//   fwd<T, MT>(), bwd_x<T, MT>(), bwd_w<T, MT>()     its __global__ symbols
//   rows_lds, w_lds, image  its LDS sizes and the floats of one partial image
//   rows<T>(call, wt, w2t), weights<T>(call, w2t, partial, splits), reduce<T>(call, partial, slots, stream)
//                           fill the argument structs from a Call and launch its reduce kernel

// the operands of an entry point, checked; w / b / dw / db: the first layer's pairs in the family's order.  forward reads
// x, w, b, w2, b2 and out = y; backward x, dy, w, b, w2, out = dx and what follows
template <int NZ> struct Call {
  const void *x, *dy, *w[NZ], *b[NZ], *w2, *b2;
  void *out, *dw[NZ], *db[NZ], *dw2, *db2, *ws;
  int64_t n;
  int c, hd, cout, act;
  bool need_dx, need_w;
};

template <typename F, typename T, int MT, bool BWD> int launch_rows(const typename F::template Rows<T> &a, hipStream_t stream) {
  const int64_t lds = F::rows_lds((int)sizeof(T), a.c, a.cout, BWD);
  ME_CHECK(lds <= kLdsBudget, "the weight chunks do not fit into LDS");
  auto fn = BWD ? F::template bwd_x<T, MT>() : F::template fwd<T, MT>();
  if (allow_lds(fn, lds) != 0) return 1;
  hipLaunchKernelGGL(fn, dim3((unsigned)ceil_div(a.n, kRows)), dim3(kThreads), (size_t)lds, stream, a);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename F, typename T, int MT> int launch_w(const typename F::template Weights<T> &a, hipStream_t stream) {
  const int64_t lds = F::w_lds((int)sizeof(T), a.c, a.cout);
  ME_CHECK(lds <= kLdsBudget, "the weight chunks and row images do not fit into LDS");
  auto fn = F::template bwd_w<T, MT>();
  if (allow_lds(fn, lds) != 0) return 1;
  hipLaunchKernelGGL(fn, dim3((unsigned)(a.hd / 32), (unsigned)a.splits), dim3(kThreads), (size_t)lds, stream, a);
  ME_LAUNCH_CHECK();
  return 0;
}

// MT = 2 | 4 | 8 register tiles for max(c, cout) / 32, up to top = the family's widest rows of the dtype / 32
#define ME_FFN_DISPATCH(top, width, ...)                                                             \
  do {                                                                                               \
    if ((width) <= 64) { constexpr int MT = 2; return __VA_ARGS__; }                                 \
    if constexpr ((top) >= 4) { if ((width) <= 128) { constexpr int MT = 4; return __VA_ARGS__; } }  \
    if constexpr ((top) >= 8) { constexpr int MT = 8; return __VA_ARGS__; }                          \
    ME_FAIL("width not served");                                                                     \
  } while (0)

template <typename F, typename T> int rows_any(const typename F::template Rows<T> &a, bool bwd, hipStream_t stream) {
  constexpr int top = (sizeof(T) == 2 ? F::kMaxBf16 : F::kMaxF32) / 32;
  const int width = std::max(a.c, a.cout);
  if (bwd) ME_FFN_DISPATCH(top, width, launch_rows<F, T, MT, true>(a, stream));
  ME_FFN_DISPATCH(top, width, launch_rows<F, T, MT, false>(a, stream));
}
template <typename F, typename T> int w_any(const typename F::template Weights<T> &a, hipStream_t stream) {
  constexpr int top = (sizeof(T) == 2 ? F::kMaxBf16 : F::kMaxF32) / 32;
  ME_FFN_DISPATCH(top, std::max(a.c, a.cout), launch_w<F, T, MT>(a, stream));
}

template <typename F> int32_t supported(int c, int hd, int cout, int elem) {
  if (elem != 2 && elem != 4) return 0;
  const int max_w = elem == 2 ? F::kMaxBf16 : F::kMaxF32;
  return (c >= 32 && c % 32 == 0 && c <= max_w && cout >= 32 && cout % 32 == 0 && cout <= max_w && hd >= 32 &&
          hd % 32 == 0) ? 1 : 0;
}

template <typename F> int32_t row_splits(int64_t n, int c, int hd, int cout, int elem) {
  if (n < 1 || supported<F>(c, hd, cout, elem) == 0) return 1;
  const int64_t blocks = ceil_div(n, kRows);
  const int64_t fill = ceil_div(kTargetGroups, hd / 32);
  // four partial images per split; together no larger than x and dy
  const int64_t cap = n * (c + cout) * elem / (16 * F::image(c, hd, cout));
  const int64_t want = std::min(blocks, std::max<int64_t>(4, std::min(fill, cap)));
  return (int32_t)ceil_div(blocks, ceil_div(blocks, want));   // no empty split
}

// the workspace of a backward call: w[i]^T [c, hd] for every i, W2^T [hd, cout], then the partial images
template <typename F> int64_t transposed_bytes(int c, int hd, int cout, int elem) {
  return align_up((F::NZ * (int64_t)c * hd + (int64_t)hd * cout) * elem, 256);
}
template <typename F> int64_t workspace_bytes(int64_t n, int c, int hd, int cout, int elem) {
  if (supported<F>(c, hd, cout, elem) == 0) return 0;
  return transposed_bytes<F>(c, hd, cout, elem) +
         4 * (int64_t)row_splits<F>(n, c, hd, cout, elem) * F::image(c, hd, cout) * (int64_t)sizeof(float);
}

// max_name: "ME_FFN_MAX_WIDTH" | "ME_GLU_MAX_WIDTH"
#define ME_FFN_CHECK_SHAPE(F, max_name, n, c, hd, cout, elem, act)                                                    \
  ME_CHECK(n >= 0 && n < (1ll << 31), "the row count must fit in int32");                                            \
  ME_CHECK(supported<F>(c, hd, cout, elem) != 0,                                                                     \
           "widths not served: c and cout multiples of 32 up to " max_name "_*, hd a multiple of 32");               \
  ME_CHECK(act >= ME_FFN_GELU && act <= ME_FFN_SILU, "unknown activation")

template <typename F, typename T> int forward(const Call<F::NZ> &m, hipStream_t stream) {
  return rows_any<F, T>(F::template rows<T>(m, nullptr, nullptr), false, stream);
}

// the transposes, the input gradient, the weight-gradient kernel and its reduce
template <typename F, typename T> int backward(const Call<F::NZ> &m, hipStream_t stream) {
  const int64_t ch = (int64_t)m.c * m.hd;
  T *wt[F::NZ], *w2t = (T *)m.ws + F::NZ * ch;   // w[i]^T [c, hd], W2^T [hd, cout]
  float *partial = (float *)((char *)m.ws + transposed_bytes<F>(m.c, m.hd, m.cout, (int)sizeof(T)));
  if (transpose<T>((const T *)m.w2, w2t, m.cout, m.hd, stream) != 0) return 1;
  if (m.need_dx) {
    for (int i = 0; i < F::NZ; ++i) {
      wt[i] = (T *)m.ws + i * ch;
      if (transpose<T>((const T *)m.w[i], wt[i], m.hd, m.c, stream) != 0) return 1;
    }
    if (rows_any<F, T>(F::template rows<T>(m, wt, w2t), true, stream) != 0) return 1;
  }
  if (!m.need_w) return 0;
  const int splits = row_splits<F>(m.n, m.c, m.hd, m.cout, (int)sizeof(T));
  if (w_any<F, T>(F::template weights<T>(m, w2t, partial, splits), stream) != 0) return 1;
  F::template reduce<T>(m, partial, 4 * splits, stream);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // namespace ffn
}  // namespace me
